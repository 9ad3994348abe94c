// vit_rowwise.h -- the kernels of the ViT encoder that walk the residual stream row by row or element by element, no matrix product:
// LayerNorm (plain and hi / lo planes), the final residual update, the tap, the CLS drop, the range scan and the zero fill, with the
// one range test of a residual update that they share with the fused-LayerNorm GEMMs (vit_gemm_wide.h, vit_gemm_ws_ln.h).  Included by
// vit.hip directly after vit_gemm_common.h, ahead of every GEMM header.
#pragma once
#include <type_traits>
#include "vit_gemm_common.h"

namespace {

// a saturated (or non-finite) residual update: the fp16 range was exceeded upstream (overflow bit 1).  Never set for bf16 operands.
template <typename T>
__device__ __forceinline__ bool update_saturated(float d0, float d1, float d2, float d3) {
    return IsF16<T>::value && !(fmaxf(fmaxf(fabsf(d0), fabsf(d1)), fmaxf(fabsf(d2), fabsf(d3))) < 65504.f);
}

// ---- LayerNorm: fp32 row -> 16-bit row (A operand of the next GEMM); one wave per token --------------------------------------
// The LayerNorm kernels keep a row in NIT float4 per lane -- four up to D = 1024 (ViT-S / B / L), six for D = 1536 (ViT-g):
// launch_layernorm; dtk_vit_forward refuses wider models.
constexpr int VIT_MAX_D = 1536;

// One row of both LayerNorm kernels.  A pending residual update (the LayerScale'd output of the previous projection / MLP of a FAST
// block, written by the GEMM epilogue; a split block adds its updates in its own epilogues) is applied here: x += delta.
// store(c, r) takes the four normalised values of columns c .. c + 3; !write: the residual update only.
template <typename T, int NIT, typename Store>
__device__ __forceinline__ void layernorm_row(float* __restrict__ x, const T* __restrict__ delta, const float* __restrict__ gam,
                                              const float* __restrict__ bet, bool write, long long rows, int D, float eps,
                                              int* __restrict__ overflow, Store store) {
    typedef typename Vec<T>::t4 T4;
    operand_mode<T>();
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    float* p = x + row * D;
    float4 v[NIT];
    float s = 0.f;
    bool sat = false;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int c = lane * 4 + it * 256;
        if (c < D) {
            v[it] = *reinterpret_cast<const float4*>(p + c);
            if (delta) {
                const T4 d = *reinterpret_cast<const T4*>(delta + row * D + c);
                const float d0 = (float)d[0], d1 = (float)d[1], d2 = (float)d[2], d3 = (float)d[3];
                sat |= update_saturated<T>(d0, d1, d2, d3);
                v[it].x += d0; v[it].y += d1; v[it].z += d2; v[it].w += d3;
                *reinterpret_cast<float4*>(p + c) = v[it];
            }
            s += (v[it].x + v[it].y) + (v[it].z + v[it].w);
        }
    }
    if (IsF16<T>::value && overflow && __any(sat) && lane == 0) atomicOr(overflow, 1);
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        if (lane * 4 + it * 256 < D) {
            const float a = v[it].x - mean, b = v[it].y - mean, cc = v[it].z - mean, d = v[it].w - mean;
            q += (a * a + b * b) + (cc * cc + d * d);
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
    if (!write) return;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int c = lane * 4 + it * 256;
        if (c < D) {
            const float4 g = *reinterpret_cast<const float4*>(gam + c), b = *reinterpret_cast<const float4*>(bet + c);
            const float r[4] = {(v[it].x - mean) * rstd * g.x + b.x, (v[it].y - mean) * rstd * g.y + b.y,
                                (v[it].z - mean) * rstd * g.z + b.z, (v[it].w - mean) * rstd * g.w + b.w};
            store(row * D + c, r);
        }
    }
}

template <typename T, int NIT = 4>
__global__ __launch_bounds__(256) void layernorm_kernel(float* __restrict__ x, const T* __restrict__ delta,
                                                        const float* __restrict__ gam, const float* __restrict__ bet,
                                                        T* __restrict__ y, long long rows, int D, float eps,
                                                        int* __restrict__ overflow) {
    typedef typename Vec<T>::t4 T4;
    layernorm_row<T, NIT>(x, delta, gam, bet, y != nullptr /* null: the final residual update only */, rows, D, eps, overflow,
                          [y](long long at, const float (&r)[4]) {
                              *reinterpret_cast<T4*>(y + at) = T4{(T)r[0], (T)r[1], (T)r[2], (T)r[3]};
                          });
}

// LayerNorm -> hi / lo planes (vit_split.h: the escalated precision)
template <typename T, int NIT = 4>
__global__ __launch_bounds__(256) void layernorm_split_kernel(float* __restrict__ x, const T* __restrict__ delta,
                                                              const float* __restrict__ gam, const float* __restrict__ bet,
                                                              T* __restrict__ y_hi, T* __restrict__ y_lo, long long rows, int D,
                                                              float eps, int* __restrict__ overflow) {
    typedef typename Vec<T>::t4 T4;
    layernorm_row<T, NIT>(x, delta, gam, bet, true, rows, D, eps, overflow, [y_hi, y_lo](long long at, const float (&r)[4]) {
        T4 h, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) { T a, b; split2<T>(r[e], a, b); h[e] = a; l[e] = b; }
        *reinterpret_cast<T4*>(y_hi + at) = h;
        *reinterpret_cast<T4*>(y_lo + at) = l;
    });
}

// y_lo null: layernorm_kernel (y null too: the residual update and its range check only); otherwise the hi / lo planes
template <typename T>
int launch_layernorm(float* x, const T* delta, const float* gam, const float* bet, T* y, T* y_lo, long long rows, int D, float eps,
                     int* ovf, hipStream_t st) {
    const dim3 grid(dtk_cdiv(rows, 4));
    auto launch = [&](auto nit) -> int {
        constexpr int NIT = decltype(nit)::value;
        if (y_lo)
            DTK_LAUNCH("vit_layernorm_split", (layernorm_split_kernel<T, NIT>), grid, dim3(256), 0, st, x, delta, gam, bet, y, y_lo, rows, D, eps, ovf);
        else
            DTK_LAUNCH("vit_layernorm", (layernorm_kernel<T, NIT>), grid, dim3(256), 0, st, x, delta, gam, bet, y, rows, D, eps, ovf);
        return DTK_OK;
    };
    return D <= 1024 ? launch(std::integral_constant<int, 4>()) : launch(std::integral_constant<int, 6>());
}

__global__ __launch_bounds__(256) void zero_kernel(uint4* __restrict__ p, long long n16) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0, 0, 0, 0);
}

// The LAST residual update of a pass, fused with what leaves the encoder (round 5): out = x + delta goes straight to tokens_out
// [F][S][D] and / or feat_out [F][S-P][D] (the P = 1 + n_registers prefix rows -- CLS and the registers -- dropped); the fp32 stream
// x is dead after the last block and is not written back.
// Replaces a statistics-free LayerNorm launch + a device copy / drop_cls pass: 2.8 GB of traffic instead of 5.0 per 90 frames.
template <typename T>
__global__ __launch_bounds__(256) void final_update_kernel(const float* __restrict__ x, const T* __restrict__ delta,
                                                           float* __restrict__ tokens_out, float* __restrict__ feat_out, int S, int D,
                                                           long long total4, int* __restrict__ overflow, int P) {
    typedef typename Vec<T>::t4 T4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool sat = false;
    if (i < total4) {
        const int d4 = D / 4;
        const long long row = i / d4;  // over F * S
        const int c = (int)(i - row * d4);
        const long long f = row / S, s = row - f * S;
        float4 v = reinterpret_cast<const float4*>(x)[i];
        const T4 d = reinterpret_cast<const T4*>(delta)[i];
        const float d0 = (float)d[0], d1 = (float)d[1], d2 = (float)d[2], d3 = (float)d[3];
        sat = update_saturated<T>(d0, d1, d2, d3);   // (the check layernorm_kernel makes)
        v.x += d0; v.y += d1; v.z += d2; v.w += d3;
        if (tokens_out) reinterpret_cast<float4*>(tokens_out)[i] = v;
        if (feat_out && s >= P) reinterpret_cast<float4*>(feat_out)[(f * (S - P) + s - P) * d4 + c] = v;
    }
    if (IsF16<T>::value && overflow && __any(sat) && (threadIdx.x & 63) == 0) atomicOr(overflow, 1);
}

// tap of the residual stream after a block (dtk_vit_model.tap_out): out += scale * (x + pending update)
template <typename T>
__global__ __launch_bounds__(256) void tap_kernel(const float* __restrict__ x, const T* __restrict__ delta, float* __restrict__ out,
                                                  float scale, long long total4) {
    typedef typename Vec<T>::t4 T4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    float4 v = reinterpret_cast<const float4*>(x)[i];
    if (delta) {
        const T4 d = reinterpret_cast<const T4*>(delta)[i];
        v.x += (float)d[0]; v.y += (float)d[1]; v.z += (float)d[2]; v.w += (float)d[3];
    }
    float4 o = reinterpret_cast<float4*>(out)[i];
    o.x += scale * v.x; o.y += scale * v.y; o.z += scale * v.z; o.w += scale * v.w;
    reinterpret_cast<float4*>(out)[i] = o;
}

// fp32 tokens [F][S][D] (CLS first, then the registers) -> token-major features [F][HW][D] (drop the P = 1 + n_registers prefix rows)
__global__ __launch_bounds__(256) void drop_cls_kernel(const float* __restrict__ x, float* __restrict__ out, int S, int D,
                                                       long long total4, int P) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int d4 = D / 4;
    const long long row = i / d4;  // over F*(S-P)
    const int c = (int)(i - row * d4);
    const long long f = row / (S - P), s = row - f * (S - P);
    reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(x)[(f * S + P + s) * d4 + c];
}

// |x| >= 65504 or non-finite anywhere in a 16-bit tensor -> *flag |= bit (DTK_VIT_CHECK_RANGE: every intermediate tensor)
template <typename T>
__global__ __launch_bounds__(256) void range_scan_kernel(const T* __restrict__ p, long long n8, int* __restrict__ flag, int bit) {
    typedef typename Vec<T>::t8 T8;
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        const T8 v = reinterpret_cast<const T8*>(p)[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) bad |= !(fabsf((float)v[e]) < 65504.f);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, bit);
}

}  // namespace
