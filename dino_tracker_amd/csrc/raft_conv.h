// raft_conv.h -- the RAFT convolution as an implicit GEMM on the matrix cores, and the all-pairs correlation on the same tile.
//
//   out[pixel][cout] = epilogue( sum over (tap, cin) of  x[pixel + tap][cin] * w[cout][tap][cin] )
//
// GEMM view: M = the output pixels of the whole batch, N = Cout, K = taps x CinPad (Cin padded to RC_K = 32 with zero weights).
// A workgroup of four waves owns RC_M = 128 pixels x 64 output channels (16 when Cout <= 16: the 256 -> 2 flow head) and walks
// K in chunks of 32: ONE tap and 32 consecutive input channels, so a chunk of the activation tile is 128 runs of 128 contiguous
// bytes of an NHWC tensor (or zeros: a tap outside the image, a row past M, a channel past Cin).  The activations are fp32 in
// memory; a thread loads four channels (16 bytes), splits them with split2 into hi + lo fp16 and stores both halves to LDS, so no
// 16-bit copy of any activation is ever written to memory and a channel SLICE of a wider tensor (pointer + channel stride) is as
// good an input as a whole tensor.  The weights are packed once, hi and lo planes [CoutPad][taps][CinPad] fp16, scaled by a power
// of two so that their lo halves stay normal numbers.
// MFMA 16x16x32 f16 as (weight tile) x (pixel tile)^T: a lane then owns four consecutive output channels of one pixel (one
// 16-byte NHWC store).  A wave computes 32 pixels x 64 channels = 8 accumulator tiles from 4 + 2 fragments per plane; split mode
// issues hi.lo, lo.hi, hi.hi (three MFMAs per term, fp32 accumulate; the dropped lo.lo term is 2^-22 relative), fp16 mode hi.hi.
// LDS rows are 32 halves padded to 40 (80 bytes): the 16 rows one 16-byte fragment read touches start in distinct bank groups.
// The next chunk's global loads are issued before the MFMAs of the current one (register prefetch, one LDS buffer).
#pragma once
#include "common.h"

namespace {

constexpr int RC_M = 128, RC_K = 32, RC_LD = 40;
typedef _Float16 rc_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 rc_h4 __attribute__((ext_vector_type(4)));
typedef float rc_f4 __attribute__((ext_vector_type(4)));

struct ConvP {
    const float* in; long long in_stride; const float* in2; long long in2_stride; int split;
    int N, H, W, Cin, Ho, Wo, KH, KW, stride, ph, pw, CinPad, Kpad;
    const _Float16 *w_hi, *w_lo; const float* bias; float inv_ws;
    float* out; long long out_stride; int Cout;
    int act; const float* res; long long res_stride; int res_relu; const float* mul; long long mul_stride; const float* gate;
    long long gate_stride;
    long long M;
    bool vec_in, vec_out;
};

// sigmoid and tanh of the epilogues.  expf / tanhf are the device library's (<= 2 ulp); the bounds in include/dtk.h (4.8e-7
// absolute) are what tests/test_gpu_raft_conv.py holds them to.
__device__ __forceinline__ float rc_activate(float v, int act) {
    if (act == DTK_RAFT_ACT_RELU) return fmaxf(v, 0.f);
    if (act == DTK_RAFT_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
    if (act == DTK_RAFT_ACT_TANH) return tanhf(v);
    return v;
}

// four fp32 values -> hi (and lo) fp16 at `row`, halves 4 g .. 4 g + 3 of an LDS tile
template <bool SPLIT>
__device__ __forceinline__ void rc_stage4(_Float16* s_hi, _Float16* s_lo, int row, int g, rc_f4 v) {
    rc_h4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        _Float16 a, b;
        split2<_Float16>(v[e], a, b);
        h[e] = a;
        l[e] = b;
    }
    *reinterpret_cast<rc_h4*>(s_hi + row * RC_LD + 4 * g) = h;
    if (SPLIT) *reinterpret_cast<rc_h4*>(s_lo + row * RC_LD + 4 * g) = l;
}

// one K chunk of the wave's 32 pixels x (16 NT) channels
template <bool SPLIT, int NT>
__device__ __forceinline__ void rc_mma(const _Float16* sW_hi, const _Float16* sW_lo, const _Float16* sX_hi, const _Float16* sX_lo,
                                       int wave, int lane, rc_f4 (&acc)[NT][2]) {
    const int r = lane & 15, ko = 8 * (lane >> 4);
    rc_h8 xh[2], xl[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int row = 32 * wave + 16 * mt + r;
        xh[mt] = *reinterpret_cast<const rc_h8*>(sX_hi + row * RC_LD + ko);
        if (SPLIT) xl[mt] = *reinterpret_cast<const rc_h8*>(sX_lo + row * RC_LD + ko);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const rc_h8 wh = *reinterpret_cast<const rc_h8*>(sW_hi + (16 * nt + r) * RC_LD + ko);
        rc_h8 wl;
        if (SPLIT) wl = *reinterpret_cast<const rc_h8*>(sW_lo + (16 * nt + r) * RC_LD + ko);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            if (SPLIT) {
                acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl[mt], acc[nt][mt], 0, 0, 0);
                acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh[mt], acc[nt][mt], 0, 0, 0);
            }
            acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh[mt], acc[nt][mt], 0, 0, 0);
        }
    }
}

template <bool SPLIT, int NT>
__global__ __launch_bounds__(256) void raft_conv_kernel(const ConvP p) {
    constexpr int BN = 16 * NT;
    __shared__ __attribute__((aligned(16))) _Float16 sX_hi[RC_M * RC_LD];
    __shared__ __attribute__((aligned(16))) _Float16 sX_lo[SPLIT ? RC_M * RC_LD : 8];
    __shared__ __attribute__((aligned(16))) _Float16 sW_hi[BN * RC_LD];
    __shared__ __attribute__((aligned(16))) _Float16 sW_lo[SPLIT ? BN * RC_LD : 8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)blockIdx.x * RC_M;
    const int n0 = blockIdx.y * BN;

    // activation staging: thread -> channel group g (4 channels) of rows rr, rr + 32, rr + 64, rr + 96
    const int g = tid & 7, rr = tid >> 3;
    int iy0[4], ix0[4];
    long long nb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long m = m0 + rr + 32 * j;
        if (m < p.M) {
            const int n = (int)(m / ((long long)p.Ho * p.Wo));
            const int rem = (int)(m - (long long)n * p.Ho * p.Wo);
            const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
            iy0[j] = oy * p.stride - p.ph;
            ix0[j] = ox * p.stride - p.pw;
            nb[j] = (long long)n * p.H * p.W;
        } else {
            iy0[j] = -(1 << 20);   // every tap falls outside: zeros
            ix0[j] = 0;
            nb[j] = 0;
        }
    }
    // weight staging: thread -> 8 halves `ws` of row `wr` of the tile (the packed planes are padded to 64 rows: no bounds)
    const int wr = tid >> 2, wseg = tid & 3;
    const bool wload = wr < BN;

    const int cpc = p.CinPad / RC_K;
    const int nchunks = p.KH * p.KW * cpc;
    rc_f4 xr[4];
    uint4 wh = {0, 0, 0, 0}, wl = {0, 0, 0, 0};

    auto load = [&](int chunk) {
        const int tap = chunk / cpc, c0 = (chunk - tap * cpc) * RC_K;
        const int ky = tap / p.KW, kx = tap - ky * p.KW;
        const int c = c0 + 4 * g;
        const float* src = p.in;
        long long cs = p.in_stride;
        int cc = c;
        if (c >= p.split) { src = p.in2; cs = p.in2_stride; cc = c - p.split; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int iy = iy0[j] + ky, ix = ix0[j] + kx;
            rc_f4 v = {0.f, 0.f, 0.f, 0.f};
            if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W && c < p.Cin) {
                const float* q = src + (nb[j] + (long long)iy * p.W + ix) * cs + cc;
                if (p.vec_in) {
                    v = *reinterpret_cast<const rc_f4*>(q);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < p.Cin) v[e] = q[e];
                }
            }
            xr[j] = v;
        }
        if (wload) {
            const size_t off = (size_t)(n0 + wr) * p.Kpad + (size_t)chunk * RC_K + 8 * wseg;
            wh = *reinterpret_cast<const uint4*>(p.w_hi + off);
            if (SPLIT) wl = *reinterpret_cast<const uint4*>(p.w_lo + off);
        }
    };

    rc_f4 acc[NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = rc_f4{0.f, 0.f, 0.f, 0.f};

    load(0);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        __syncthreads();   // the previous chunk's fragments have been read
#pragma unroll
        for (int j = 0; j < 4; ++j) rc_stage4<SPLIT>(sX_hi, sX_lo, rr + 32 * j, g, xr[j]);
        if (wload) {
            *reinterpret_cast<uint4*>(sW_hi + wr * RC_LD + 8 * wseg) = wh;
            if (SPLIT) *reinterpret_cast<uint4*>(sW_lo + wr * RC_LD + 8 * wseg) = wl;
        }
        __syncthreads();
        if (chunk + 1 < nchunks) load(chunk + 1);
        rc_mma<SPLIT, NT>(sW_hi, sW_lo, sX_hi, sX_lo, wave, lane, acc);
    }

    // epilogue: lane -> pixel (lane & 15) of each pixel tile, channels 4 (lane >> 4) .. + 3 of each channel tile
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const long long m = m0 + 32 * wave + 16 * mt + (lane & 15);
        if (m >= p.M) continue;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int c = n0 + 16 * nt + 4 * (lane >> 4);
            if (c >= p.Cout) continue;
            const bool full = p.vec_out && c + 4 <= p.Cout;
            float* o = p.out + m * p.out_stride + c;
            rc_f4 v = acc[nt][mt], hprev = {0.f, 0.f, 0.f, 0.f}, z = hprev, r = hprev, ml = {1.f, 1.f, 1.f, 1.f};
            if (full) {
                if (p.gate) { z = *reinterpret_cast<const rc_f4*>(p.gate + m * p.gate_stride + c); hprev = *reinterpret_cast<const rc_f4*>(o); }
                if (p.mul) ml = *reinterpret_cast<const rc_f4*>(p.mul + m * p.mul_stride + c);
                if (p.res) r = *reinterpret_cast<const rc_f4*>(p.res + m * p.res_stride + c);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < p.Cout) {
                        if (p.gate) { z[e] = p.gate[m * p.gate_stride + c + e]; hprev[e] = o[e]; }
                        if (p.mul) ml[e] = p.mul[m * p.mul_stride + c + e];
                        if (p.res) r[e] = p.res[m * p.res_stride + c + e];
                    }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = v[e] * p.inv_ws + (c + e < p.Cout ? p.bias[c + e] : 0.f);
                t = rc_activate(t, p.act);
                if (p.mul) t = t * ml[e];
                if (p.gate) t = (1.0f - z[e]) * hprev[e] + z[e] * t;
                if (p.res) { t = t + r[e]; if (p.res_relu) t = fmaxf(t, 0.f); }
                v[e] = t;
            }
            if (full) {
                *reinterpret_cast<rc_f4*>(o) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < p.Cout) o[e] = v[e];
            }
        }
    }
}

// fp32 weights [Cout][Cin][KH][KW] -> hi / lo planes [CoutPad][KH KW][CinPad] of w * wscale, zeros in the padding
__global__ void raft_conv_pack_kernel(const float* __restrict__ w, int cout, int cin, int kh, int kw, int cin_pad, long long total,
                                      float wscale, _Float16* __restrict__ hi, _Float16* __restrict__ lo) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % cin_pad);
    const int tap = (int)((i / cin_pad) % (kh * kw));
    const int o = (int)(i / ((long long)cin_pad * kh * kw));
    float v = 0.f;
    if (o < cout && c < cin) v = w[((size_t)o * cin + c) * kh * kw + tap] * wscale;
    _Float16 a, b;
    split2<_Float16>(v, a, b);
    hi[i] = a;
    lo[i] = b;
}

// ---- all-pairs correlation: corr[n][i][j] = <f1[n][i], f2[n][j]> * scale, both operands fp32 rows [cell][C], split on the way in
struct CorrP {
    const float *f1, *f2;
    float* out;
    int hw, C;
    float scale;
};

template <bool SPLIT>
__global__ __launch_bounds__(256) void raft_corr_kernel(const CorrP p) {
    constexpr int NT = 4, BN = 64;
    __shared__ __attribute__((aligned(16))) _Float16 sX_hi[RC_M * RC_LD];
    __shared__ __attribute__((aligned(16))) _Float16 sX_lo[SPLIT ? RC_M * RC_LD : 8];
    __shared__ __attribute__((aligned(16))) _Float16 sW_hi[BN * RC_LD];
    __shared__ __attribute__((aligned(16))) _Float16 sW_lo[SPLIT ? BN * RC_LD : 8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * RC_M, j0 = blockIdx.y * BN, n = blockIdx.z;
    const float* f1 = p.f1 + (size_t)n * p.hw * p.C;
    const float* f2 = p.f2 + (size_t)n * p.hw * p.C;
    const int g = tid & 7, rr = tid >> 3;
    rc_f4 xr[4], wr2[2];
    auto load = [&](int chunk) {
        const int c = chunk * RC_K + 4 * g;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + rr + 32 * j;
            xr[j] = i < p.hw ? *reinterpret_cast<const rc_f4*>(f1 + (size_t)i * p.C + c) : rc_f4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int jj = j0 + rr + 32 * j;
            wr2[j] = jj < p.hw ? *reinterpret_cast<const rc_f4*>(f2 + (size_t)jj * p.C + c) : rc_f4{0.f, 0.f, 0.f, 0.f};
        }
    };
    rc_f4 acc[NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = rc_f4{0.f, 0.f, 0.f, 0.f};
    const int nchunks = p.C / RC_K;
    load(0);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) rc_stage4<SPLIT>(sX_hi, sX_lo, rr + 32 * j, g, xr[j]);
#pragma unroll
        for (int j = 0; j < 2; ++j) rc_stage4<SPLIT>(sW_hi, sW_lo, rr + 32 * j, g, wr2[j]);
        __syncthreads();
        if (chunk + 1 < nchunks) load(chunk + 1);
        rc_mma<SPLIT, NT>(sW_hi, sW_lo, sX_hi, sX_lo, wave, lane, acc);
    }
    float* out = p.out + (size_t)n * p.hw * p.hw;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int i = i0 + 32 * wave + 16 * mt + (lane & 15);
        if (i >= p.hw) continue;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int j = j0 + 16 * nt + 4 * (lane >> 4);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e < p.hw) out[(size_t)i * p.hw + j + e] = acc[nt][mt][e] * p.scale;
        }
    }
}

}  // namespace
