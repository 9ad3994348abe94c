// vit.hip -- P1: DINOv2 ViT encoder as driven by VitExtractor (models/extractor.py:41-150, utils.py:33-72):
// overlapping patch embedding (14x14, stride 7) of ImageNet-normalised frames + interpolated position encoding,
// `depth` transformer blocks (LN -> QKV -> MHSA -> proj -> LayerScale -> +res; LN -> fc1 -> GELU -> fc2 -> LayerScale
// -> +res; ViT-g/14: LN -> w12 -> silu(gate) * value -> w3 instead, dtk_vit_model.ffn), output = residual stream after the last requested block (no final norm), CLS included.
//
//   patch_embed_kernel  exact fp32 implicit GEMM on the f32-input MFMA (K = 3*14*14 = 588), mean/std fused in the load
//   layernorm_kernel    one wave per token, fp32 statistics, 16-bit output; the row in NIT float4 per lane (D <= 1024: 4, D <= 1536: 6)
//   gemm_tiled_kernel   (vit_gemm_tiled.h) C = A W^T on MFMA 16x16x32 (fp32 accumulate), 128x128 tiles, LDS double-buffered, with
//                       fused epilogues: QKV split (Q pre-scaled by log2(e)/sqrt(d), V written transposed), GELU,
//                       LayerScale + residual add into the fp32 stream.  The forms the blocks run on: vit_gemm_ws.h (K = 384,
//                       weight-stationary), vit_gemm_ws_ln.h (the attention projection at D = 384 with LayerNorm-2), vit_gemm_wide.h (LDS-DMA pipelines), vit_split.h (the escalated precision);
//                       launch_gemm / launch_gemm_split below choose among them.
//   attention4_kernel   (vit_attention4.h; round 4) flash attention, d_head = 64: S^T = K Q^T and O^T = V^T P^T on MFMA 32x32x16
//                       so that every per-query quantity is lane-local; K / V^T tiles by LDS-DMA into XOR-swizzled images;
//                       ONE wave per SIMD with 64 queries, its two query tiles half a key tile out of phase (the softmax of
//                       one runs under the MFMAs of the other), fragments held in registers for both; exp2-domain softmax
//                       with optimistic exponentials (guarded); XCD-aware grid.  The one fallback / cross-check
//                       (DTK_VIT_ATTENTION_V4) since round 6.
//   attention6_kernel   (vit_attention6.h; round 6) the same arithmetic, tile layout and guards with 128 queries per wave: what
//                       dtk_vit_forward runs.  (The round 2-3 kernel lives on in scripts/ubench/ for the micro-benchmark only.)
// Residual stream fp32.  Matrix operands (LN output, Q / K / V^T / P, attention output, MLP hidden, the pending residual
// update, the weights) are a template parameter T: _Float16 by default since round 3 -- the same MFMA rate as bf16 with
// 8x less operand rounding (fp16 range: activations saturate at +-65504, FP16_OVFL mode, and set the model's overflow
// word) -- or __bf16 with DTK_VIT_BF16 (the reference runs fp32; parity is stated in DESIGN.md section 4).
#include <stdlib.h>
#include "common.h"
#include "vit_attention4.h"
#include "vit_attention6.h"
#include "vit_gemm_common.h"
#include "vit_gemm_tiled.h"
#include "vit_gemm_ws.h"
#include "vit_gemm_ws_ln.h"
#include "vit_gemm_wide.h"
#include "vit_split.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// patch embedding: tokens[f][1 + r*pw + c][:] = W . patch(r,c) + b + pos[r*pw + c];  tokens[f][0] = cls_pos
// 32 patches x 32 output features per wave (MFMA 32x32x2 f32), 4 waves = 64 patches x 64 features per workgroup
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void patch_embed_kernel(const float* __restrict__ frames, const float* __restrict__ Wp,
                                                          const float* __restrict__ bp, const float* __restrict__ pos,
                                                          const float* __restrict__ cls_pos,
                                                          const float* __restrict__ mean_std, float* __restrict__ x,
                                                          int H, int W, int ph, int pw, int D, int patch, int stride,
                                                          int S) {
    const int HW = ph * pw;
    const int K = 3 * patch * patch;
    const int frame = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int p0 = blockIdx.x * 64 + (w >> 1) * 32;
    const int n0 = blockIdx.y * 64 + (w & 1) * 32;
    const int li = lane & 31, lk = lane >> 5;
    const float* img = frames + (size_t)frame * 3 * H * W;
    const int p = min(p0 + li, HW - 1);
    const int pr = p / pw, pc = p % pw;
    const int n = min(n0 + li, D - 1);
    const float* wrow = Wp + (size_t)n * K;  // [D][3][patch][patch]
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k = lk; k < K; k += 2) {
        const int ch = k / (patch * patch), rem = k - ch * patch * patch;
        const int ky = rem / patch, kx = rem - ky * patch;
        const float px = img[((size_t)ch * H + pr * stride + ky) * W + pc * stride + kx];
        const float a = (px - mean_std[ch]) / mean_std[3 + ch];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wrow[k], acc, 0, 0, 0);
    }
    const int co = n0 + li;
    if (co < D) {
        const float b = bp[co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * lk;
            const int pp = p0 + i;
            if (pp < HW) x[((size_t)frame * S + 1 + pp) * D + co] = acc[r] + b + pos[(size_t)pp * D + co];
        }
    }
    if (blockIdx.x == 0 && (w >> 1) == 0 && lk == 0 && co < D) x[(size_t)frame * S * D + co] = cls_pos[co];
}

// ---------------------------------------------------------------------------------------------------------------
// patch embedding on the split-fp16 MFMA (patch 14, stride 7): fp32-grade results from fp16 matrix instructions.
// Every fp32 operand is carried as hi + lo fp16 halves and a product is xh.wh + xh.wl + xl.wh accumulated in fp32 (each
// fp16 x fp16 product is exact in fp32; the dropped xl.wl term is 2^-22 relative).  The normalised frame is first
// rewritten as two NHWC planes with 4 channels per pixel (channel 3 = 0), so that with k = (ky * 14 + kx) * 4 + c an
// 8-wide A fragment is two neighbouring taps = two 8-byte LDS reads -- no im2col gather.  A workgroup owns 128
// consecutive tokens of one patch row (a wave 32 of them) x 96 output features and walks K = 784 in seven chunks of two
// kernel rows; per chunk the two pixel rows (903 px) and the 96 x 112 weight slab (both planes) are staged in LDS.
// ---------------------------------------------------------------------------------------------------------------
constexpr int PE_P = 14, PE_S = 7, PE_TOK = 128, PE_NF = 96;
constexpr int PE_ROWPX = (PE_TOK - 1) * PE_S + PE_P;  // 903 pixels of one kernel row for 128 tokens
constexpr int PE_K = PE_P * PE_P * 4;                 // 784
constexpr int PE_CK = 2 * PE_P * 4;                   // 112 k per chunk (two kernel rows)
constexpr int PE_WP = PE_CK + 8;                      // weight row pitch in halves (240 B: conflict-free fragments)
constexpr float PE_WSCALE = 256.f;                    // weights carry 2^8 so that their lo halves stay normal numbers

__global__ __launch_bounds__(256) void frame_split4_kernel(const float* __restrict__ frames, const float* __restrict__ mean_std,
                                                           h4v* __restrict__ hi_, h4v* __restrict__ lo_, int H, int W,
                                                           long long npix) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // over frames * H * W
    if (i >= npix) return;
    const long long f = i / ((long long)H * W), p = i - f * (long long)H * W;
    const float* fr = frames + f * 3 * (long long)H * W + p;
    h4v h, l;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = (fr[(long long)c * H * W] - mean_std[c]) / mean_std[3 + c];
        h[c] = (half_t)v;
        l[c] = (half_t)(v - (float)h[c]);
    }
    h[3] = (half_t)0.f;
    l[3] = (half_t)0.f;
    hi_[i] = h;
    lo_[i] = l;
}

// [D][3][14][14] fp32 -> split planes [D][784] of w * 2^8, k = (ky * 14 + kx) * 4 + c
__global__ void pack_patch_split_kernel(const float* __restrict__ w, int D, half_t* __restrict__ Wh, half_t* __restrict__ Wl) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)D * PE_K) return;
    const int n = (int)(idx / PE_K), k = (int)(idx - (long long)n * PE_K);
    const int tap = k >> 2, c = k & 3;
    const float v = c < 3 ? w[((size_t)n * 3 + c) * (PE_P * PE_P) + tap] * PE_WSCALE : 0.f;
    const half_t h = (half_t)v;
    Wh[idx] = h;
    Wl[idx] = (half_t)(v - (float)h);
}

__global__ __launch_bounds__(256) void patch_embed_split_kernel(const h4v* __restrict__ in_hi, const h4v* __restrict__ in_lo,
                                                                const half_t* __restrict__ Wh, const half_t* __restrict__ Wl,
                                                                const float* __restrict__ bp, const float* __restrict__ pos,
                                                                const float* __restrict__ cls_pos, float* __restrict__ x,
                                                                int H, int W, int ph, int pw, int D, int S, int groups_x,
                                                                int units, int slabs) {
    __shared__ h4v Xh[2 * PE_ROWPX], Xl[2 * PE_ROWPX];
    __shared__ __attribute__((aligned(16))) half_t Wsh[PE_NF * PE_WP], Wsl[PE_NF * PE_WP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // Block -> (frame, patch row, token group, feature slab).  Workgroup b runs on XCD b % 8 and every XCD has its own L2:
    // the feature slabs of a token group re-read the same pixel rows, and so does the patch row below it (stride 7, kernel
    // 14), so each XCD gets a contiguous range of (frame, patch row, group) units and runs a unit's slabs back to back --
    // with the plain 3-D grid those blocks sat on different XCDs and every re-read went to HBM (PMC: 7.5 GB fetched per
    // 90-frame launch for 0.6 GB of split frames).
    const int per_xcd = (units + 7) / 8;
    const int within = blockIdx.x >> 3;
    const int unit = (blockIdx.x & 7) * per_xcd + within / slabs;
    if (within / slabs >= per_xcd || unit >= units) return;
    const int n0 = (within % slabs) * PE_NF;
    const int pc0 = (unit % groups_x) * PE_TOK, pr = (unit / groups_x) % ph;
    const size_t frame = unit / (groups_x * ph);
    const int li = lane & 31, hh = lane >> 5;
    const h4v* fh = in_hi + frame * (size_t)H * W;
    const h4v* fl = in_lo + frame * (size_t)H * W;
    const int tokl = w * 32 + li;  // this lane's token (row of the A operand) inside the group
    f16v acc[3];
#pragma unroll
    for (int n = 0; n < 3; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    for (int c = 0; c < PE_P / 2; ++c) {
        __syncthreads();
        for (int idx = tid; idx < 2 * PE_ROWPX; idx += 256) {
            const int r = idx / PE_ROWPX, px = idx - r * PE_ROWPX;
            const size_t g = (size_t)(pr * PE_S + 2 * c + r) * W + min(pc0 * PE_S + px, W - 1);
            Xh[idx] = fh[g];
            Xl[idx] = fl[g];
        }
        for (int idx = tid; idx < PE_NF * (PE_CK / 8); idx += 256) {
            const int f = idx / (PE_CK / 8), piece = idx - f * (PE_CK / 8);
            const size_t src = (size_t)min(n0 + f, D - 1) * PE_K + c * PE_CK + piece * 8;
            *reinterpret_cast<uint4*>(Wsh + f * PE_WP + piece * 8) = *reinterpret_cast<const uint4*>(Wh + src);
            *reinterpret_cast<uint4*>(Wsl + f * PE_WP + piece * 8) = *reinterpret_cast<const uint4*>(Wl + src);
        }
        __syncthreads();
#pragma unroll
        for (int ls = 0; ls < PE_CK / 16; ++ls) {
            const int t0 = 2 * (2 * ls + hh);  // first of this lane's two taps inside the chunk (kx even: same row)
            const int p0 = (t0 / PE_P) * PE_ROWPX + tokl * PE_S + t0 % PE_P;
            const h4v a0 = Xh[p0], a1 = Xh[p0 + 1], b0 = Xl[p0], b1 = Xl[p0 + 1];
            const h8 xh = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
            const h8 xl = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const int wo = (n * 32 + li) * PE_WP + ls * 16 + hh * 8;
                const h8 wh = *reinterpret_cast<const h8*>(Wsh + wo), wl = *reinterpret_cast<const h8*>(Wsl + wo);
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, wh, acc[n], 0, 0, 0);
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wl, acc[n], 0, 0, 0);
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wh, acc[n], 0, 0, 0);
            }
        }
    }
    // D[i][j]: j = lane & 31 (feature), i = (r&3) + 8 (r>>2) + 4 hh (token of the wave's 32)
#pragma unroll
    for (int n = 0; n < 3; ++n) {
        const int co = n0 + n * 32 + li;
        if (co >= D) continue;
        const float b = bp[co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int pc = pc0 + w * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (pc < pw) {
                const int pp = pr * pw + pc;
                x[((size_t)frame * S + 1 + pp) * D + co] = acc[n][r] * (1.f / PE_WSCALE) + b + pos[(size_t)pp * D + co];
            }
        }
        if (pr == 0 && pc0 == 0 && w == 0 && hh == 0) x[(size_t)frame * S * D + co] = cls_pos[co];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm: fp32 row -> bf16 row (A operand of the next GEMM); one wave per token
// ---------------------------------------------------------------------------------------------------------------
template <typename T, int NIT = 4>
__global__ __launch_bounds__(256) void layernorm_kernel(float* __restrict__ x, const T* __restrict__ delta,
                                                        const float* __restrict__ gam, const float* __restrict__ bet,
                                                        T* __restrict__ y, long long rows, int D, float eps,
                                                        int* __restrict__ overflow) {
    typedef typename Vec<T>::t8 T8;
    typedef typename Vec<T>::t4 T4;
    (void)sizeof(T8); (void)sizeof(T4);
    operand_mode<T>();
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    float* p = x + row * D;
    // the row stays in registers (NIT float4 per lane: four for D <= 1024, six for D <= 1536 -- launch_layernorm); a pending residual update (the LayerScale'd output of
    // the previous projection / MLP, written by the GEMM epilogue) is applied here: x += delta
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
                // a saturated (or non-finite) residual update: the fp16 range was exceeded upstream
                if (IsF16<T>::value) sat |= !(fmaxf(fmaxf(fabsf(d0), fabsf(d1)), fmaxf(fabsf(d2), fabsf(d3))) < 65504.f);
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
    if (!y) return;  // final residual update only
    T* o = y + row * D;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int c = lane * 4 + it * 256;
        if (c < D) {
            const float4 g = *reinterpret_cast<const float4*>(gam + c), b = *reinterpret_cast<const float4*>(bet + c);
            T4 r = {(T)((v[it].x - mean) * rstd * g.x + b.x), (T)((v[it].y - mean) * rstd * g.y + b.y),
                     (T)((v[it].z - mean) * rstd * g.z + b.z), (T)((v[it].w - mean) * rstd * g.w + b.w)};
            *reinterpret_cast<T4*>(o + c) = r;
        }
    }
}

__global__ __launch_bounds__(256) void zero_kernel(uint4* __restrict__ p, long long n16) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0, 0, 0, 0);
}

// The LAST residual update of a pass, fused with what leaves the encoder (round 5): out = x + delta goes straight to tokens_out
// [F][S][D] and / or feat_out [F][S-1][D] (CLS dropped); the fp32 stream x is dead after the last block and is not written back.
// Replaces a statistics-free LayerNorm launch + a device copy / drop_cls pass: 2.8 GB of traffic instead of 5.0 per 90 frames.
template <typename T>
__global__ __launch_bounds__(256) void final_update_kernel(const float* __restrict__ x, const T* __restrict__ delta,
                                                           float* __restrict__ tokens_out, float* __restrict__ feat_out, int S, int D,
                                                           long long total4, int* __restrict__ overflow) {
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
        // a saturated (or non-finite) residual update: the fp16 range was exceeded upstream (the check layernorm_kernel makes)
        if (IsF16<T>::value) sat = !(fmaxf(fmaxf(fabsf(d0), fabsf(d1)), fmaxf(fabsf(d2), fabsf(d3))) < 65504.f);
        v.x += d0; v.y += d1; v.z += d2; v.w += d3;
        if (tokens_out) reinterpret_cast<float4*>(tokens_out)[i] = v;
        if (feat_out && s > 0) reinterpret_cast<float4*>(feat_out)[(f * (S - 1) + s - 1) * d4 + c] = v;
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

// fp32 tokens [F][S][D] (CLS first) -> token-major features [F][HW][D] (drop CLS)
__global__ __launch_bounds__(256) void drop_cls_kernel(const float* __restrict__ x, float* __restrict__ out, int S, int D,
                                                       long long total4) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int d4 = D / 4;
    const long long row = i / d4;  // over F*(S-1)
    const int c = (int)(i - row * d4);
    const long long f = row / (S - 1), s = row - f * (S - 1);
    reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(x)[(f * S + 1 + s) * d4 + c];
}

// Frames per pass of the encoder: large batches give the weight-stationary GEMMs long token chunks per workgroup (their weights
// are loaded once per chunk).  Round 4: 90 (a whole benchmark video: 7.8 GB of activations, 2.7 % of the 288 GB) instead of
// 30 -- fewer, longer launches: the attention's last partial round of workgroups weighs 0.7 % instead of 2.2 %, the
// weight-stationary GEMMs load their weights a third as often; 301.4 -> 294.8 ms per step (profiles/r04_frame_batch_sweep.txt).
constexpr int VIT_FRAME_BATCH = 90;

struct VitPlan {
    int S, Sp, FB;
    size_t x, xn, q, k, vt, ao, hid, delta, total;
    bool split;                                    // some block runs on split operands (dtk_vit_layer.qkv_w_lo): the lo planes exist
    size_t xn_lo, q_lo, k_lo, vt_lo, ao_lo, hid_lo;
};

inline bool vit_layer_split(const dtk_vit_layer& L) { return L.qkv_w_lo != nullptr; }

VitPlan vit_plan(const dtk_vit_model* m, int ph, int pw, int frames) {
    VitPlan p;
    p.S = ph * pw + 1;
    p.Sp = (p.S + 127) / 128 * 128;
    const int fb = m->frame_batch > 0 ? m->frame_batch : VIT_FRAME_BATCH;
    p.FB = frames < fb ? frames : fb;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t off = 0;
    const size_t rows = (size_t)p.FB * p.S;
    p.x = off; off = al(off + rows * m->D * 4);
    p.xn = off; off = al(off + rows * m->D * 2);
    p.q = off; off = al(off + (size_t)p.FB * m->heads * p.Sp * 64 * 2);
    p.k = off; off = al(off + (size_t)p.FB * m->heads * p.Sp * 64 * 2);
    p.vt = off; off = al(off + (size_t)p.FB * m->heads * p.Sp * 64 * 2);
    p.ao = off; off = al(off + rows * m->D * 2);
    p.hid = off; off = al(off + rows * 4 * m->D * 2);
    p.delta = off; off = al(off + rows * m->D * 2);
    p.split = false;
    for (int l = 0; l < m->depth; ++l) p.split |= vit_layer_split(m->layers[l]);
    p.xn_lo = p.q_lo = p.k_lo = p.vt_lo = p.ao_lo = p.hid_lo = 0;
    if (p.split) {   // the lo planes of a split block's operands (same shapes as the hi planes; q / k / vt contiguous: zeroed together)
        p.xn_lo = off; off = al(off + rows * m->D * 2);
        p.q_lo = off; off = al(off + (size_t)p.FB * m->heads * p.Sp * 64 * 2);
        p.k_lo = off; off = al(off + (size_t)p.FB * m->heads * p.Sp * 64 * 2);
        p.vt_lo = off; off = al(off + (size_t)p.FB * m->heads * p.Sp * 64 * 2);
        p.ao_lo = off; off = al(off + rows * m->D * 2);
        p.hid_lo = off; off = al(off + rows * 4 * m->D * 2);
    }
    p.total = off;
    return p;
}

// attention launch (vit_run, dtk_vit_attention): attention6, or with v4 (DTK_VIT_ATTENTION_V4 / DTK_OPERAND_ATTENTION_V4) attention4
// (rounds 4-5: 64 queries per wave), the fallback / cross-check.
template <typename T>
int attention_launch(const T* q, const T* k, const T* vt, T* o, int S, int Sp, int heads, int D, int FH, bool v4, hipStream_t st) {
    int QB;
    if (v4) {
        const unsigned grid = attn::attention_grid(FH, S, 256, &QB);
        DTK_LAUNCH("vit_attention", (attn::attention4_kernel<T, 0>), dim3(grid), dim3(256), 0, st, q, k, vt, o, S, Sp, heads, D,
                   FH, QB);
    } else {
        const unsigned grid = attn::attention_grid(FH, S, 128 * attn::A6_NQ, &QB);
        DTK_LAUNCH("vit_attention", (attn::attention6_kernel<T, 0>), dim3(grid), dim3(256), 0, st, q, k, vt, o, S, Sp, heads, D,
                   FH, QB);
    }
    return DTK_OK;
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

// The LayerNorm launches of vit_run: the kernels keep a row in NIT float4 per lane -- four up to D = 1024 (the code of ViT-S / B / L,
// unchanged), six for D = 1536 (ViT-g); dtk_vit_forward refuses wider models.
constexpr int VIT_MAX_D = 1536;
template <typename T>
int launch_layernorm(float* x, const T* delta, const float* gam, const float* bet, T* y, long long rows, int D, float eps, int* ovf,
                     hipStream_t st) {
    if (D <= 1024)
        DTK_LAUNCH("vit_layernorm", (layernorm_kernel<T, 4>), dim3(dtk_cdiv(rows, 4)), dim3(256), 0, st, x, delta, gam, bet, y, rows, D, eps, ovf);
    else
        DTK_LAUNCH("vit_layernorm", (layernorm_kernel<T, 6>), dim3(dtk_cdiv(rows, 4)), dim3(256), 0, st, x, delta, gam, bet, y, rows, D, eps, ovf);
    return DTK_OK;
}
template <typename T>
int launch_layernorm_split(float* x, const T* delta, const float* gam, const float* bet, T* y_hi, T* y_lo, long long rows, int D,
                           float eps, int* ovf, hipStream_t st) {
    if (D <= 1024)
        DTK_LAUNCH("vit_layernorm_split", (layernorm_split_kernel<T, 4>), dim3(dtk_cdiv(rows, 4)), dim3(256), 0, st, x, delta, gam, bet, y_hi,
                   y_lo, rows, D, eps, ovf);
    else
        DTK_LAUNCH("vit_layernorm_split", (layernorm_split_kernel<T, 6>), dim3(dtk_cdiv(rows, 4)), dim3(256), 0, st, x, delta, gam, bet, y_hi,
                   y_lo, rows, D, eps, ovf);
    return DTK_OK;
}

// Which kernels the GEMMs of a pass run on: decided once from the model width D and dtk_vit_model.flags (NOT from a GEMM's own K).
struct GemmPath {
    bool tiled;    // DTK_VIT_TILED_GEMMS: every GEMM on the register-staged 128 x 128 kernels (the tests' cross-check)
    bool ws;       // D = 384: the K = 384 GEMMs weight-stationary, fc2 on gemm_wide_delta_kernel
    bool wide;     // D a multiple of 256: the 256 x 256 LDS-DMA kernel
    bool ws_v1;    // DTK_VIT_GEMM_WS_V1: the round 1-3 form of the weight-stationary kernel (A / B)
    bool wide_v1;  // DTK_VIT_GEMM_WIDE_V1: the LDS-DMA kernels (split one included) without half-step prefetch / staged epilogues (A / B)
    bool fc2_ln;   // fc2 of a block may carry the next block's LayerNorm-1 (vit_run: when that block exists and is a fast one)
    bool proj_ln;  // the attention projection carries its block's LayerNorm-2 (gemm_ws_ln_kernel); every A / B switch turns it off
};
inline GemmPath gemm_path(int D, int f) {
    const bool tiled = (f & DTK_VIT_TILED_GEMMS) != 0, ws = !tiled && D == WS_K, wide_v1 = (f & DTK_VIT_GEMM_WIDE_V1) != 0;
    static_assert(WS_K == WD_N, "fc2 of the weight-stationary width is gemm_wide_delta_kernel's shape");
    const bool ws_v1 = (f & DTK_VIT_GEMM_WS_V1) != 0, fc2_ln = ws && !wide_v1 && !(f & DTK_VIT_NO_LN_FUSION);
    return {tiled, ws, !tiled && D % W2_N == 0, ws_v1, wide_v1, fc2_ln, fc2_ln && !ws_v1};
}
inline GemmPath gemm_path(const dtk_vit_model* m) { return gemm_path(m->D, m->flags); }

// One GEMM of a fast block, C[rows][N] = A[rows][K] . W[N][K]^T with epilogue EPI.  First match wins:
//
//   EPI_F32 (the qkv facet)             gemm_tiled_kernel<T, EPI_F32>, always
//   path.ws, N = K = 384, e.ln_out set  gemm_ws_ln_kernel<T>             (proj + LayerNorm-2)           gemm_ws_ln_grid     x 256
//   path.ws, K = 384 (qkv, proj, fc1)   gemm_ws_kernel<T, EPI>            (ws_v1: <T, EPI, 0>)           gemm_ws_grid(N)     x 256
//                                       (not the qkv of SEVERAL frames shorter than its 32-row tile, S < 32: those fall through to the last line)
//   path.ws, K != 384 (fc2: N = 384)    gemm_wide_delta_kernel<T>         (wide_v1: <T, false>;          rows / 256          x 512
//                                                                          e.ln_out set: <T, true, true>)
//   path.wide                           gemm_wide_kernel<T, EPI>          (wide_v1: <T, EPI, false>)     gemm_wide_grid(N)   x 512
//   otherwise                           gemm_tiled_kernel<T, EPI>                                        gemm_grid(N)        x 256
// (EPI_SWIGLU, the w12 GEMM of ViT-g, has its own two-line launcher below: launch_gemm_swiglu.)
//
// (path.ws and path.wide exclude each other: 384 is not a multiple of 256.  The caller sets e.ln_* only under path.fc2_ln (fc2) /
//  path.proj_ln (proj).)
template <typename T, int EPI>
int launch_gemm(const char* name, const GemmPath& path, const T* A, const T* W, long long rows, int N, int K, const GemmEpi<T>& e,
                hipStream_t st) {
    if constexpr (EPI != EPI_F32) {
        // (gemm_ws_kernel's QKV epilogue steps (frame, position) a tile at a time and lets a tile cross ONE frame end: S >= WS_ROWS.
        //  SEVERAL shorter frames -- under 49 x 49 pixels -- put Q / K rows into the padding of the wrong frame; the tiled kernel divides
        //  per row.)
        const bool ws_fits = EPI != EPI_QKV || e.S >= WS_ROWS || rows <= e.S;
        if constexpr (EPI == EPI_DELTA) {
            if (path.ws && K == WS_K && N == WS_K && e.ln_out) {
                const auto gr = gemm_ws_ln_grid(rows);
                DTK_LAUNCH(name, (gemm_ws_ln_kernel<T>), gr.first, dim3(256), 0, st, A, W, rows, e, gr.second);
                return DTK_OK;
            }
        }
        if (path.ws && K == WS_K && ws_fits) {
            const auto gr = gemm_ws_grid(N, rows);
            // (the hand-cut form of gemm_ws_kernel gives a wave all of its 64 columns or none: N = 3 D, D, 4 D with D = 384)
            if (path.ws_v1)
                DTK_LAUNCH(name, (gemm_ws_kernel<T, EPI, 0>), gr.first, dim3(256), 0, st, A, W, rows, N, e, gr.second);
            else if (N % 64 != 0 || DTK_DBG(e.no_store, 128))   // (DTK_DEV bit 128: the form before the hand-cut step, for A / B)
                DTK_LAUNCH(name, (gemm_ws_kernel<T, EPI, 3, false>), gr.first, dim3(256), 0, st, A, W, rows, N, e, gr.second);
            else
                DTK_LAUNCH(name, (gemm_ws_kernel<T, EPI>), gr.first, dim3(256), 0, st, A, W, rows, N, e, gr.second);
            return DTK_OK;
        }
        if (path.ws && EPI == EPI_DELTA) {   // (not a template of EPI: no instantiation is added by the other epilogues' launchers)
            const dim3 grid(dtk_cdiv(rows, WD_M));
            if (path.wide_v1)
                DTK_LAUNCH(name, (gemm_wide_delta_kernel<T, false>), grid, dim3(512), 0, st, A, W, rows, K, e);
            else if (e.ln_out)
                DTK_LAUNCH(name, (gemm_wide_delta_kernel<T, true, true>), grid, dim3(512), 0, st, A, W, rows, K, e);
            else
                DTK_LAUNCH(name, (gemm_wide_delta_kernel<T, true>), grid, dim3(512), 0, st, A, W, rows, K, e);
            return DTK_OK;
        }
        if (path.wide) {
            const dim3 grid(gemm_wide_grid(N, rows));
            if (path.wide_v1)
                DTK_LAUNCH(name, (gemm_wide_kernel<T, EPI, false>), grid, dim3(512), 0, st, A, W, rows, N, K, e);
            else
                DTK_LAUNCH(name, (gemm_wide_kernel<T, EPI, true>), grid, dim3(512), 0, st, A, W, rows, N, K, e);
            return DTK_OK;
        }
    }
    DTK_LAUNCH(name, (gemm_tiled_kernel<T, EPI>), dim3(gemm_grid(N, rows)), dim3(256), 0, st, A, W, rows, N, K, e);
    return DTK_OK;
}

// The w12 GEMM of a SwiGLU block (ViT-g: D = 1536, N = 2 x 4096 packed rows, EPI_SWIGLU): gemm_wide_kernel<T, EPI_SWIGLU> (path.wide:
// 1536 is a multiple of 256) or, DTK_VIT_TILED_GEMMS, gemm_tiled_kernel<T, EPI_SWIGLU>.  There is no *_V1 form: vit_swiglu_flags_ok.
template <typename T>
int launch_gemm_swiglu(const char* name, const GemmPath& path, const T* A, const T* W, long long rows, int N, int K, const GemmEpi<T>& e,
                       hipStream_t st) {
    if (path.wide)
        DTK_LAUNCH(name, (gemm_wide_kernel<T, EPI_SWIGLU, true>), dim3(gemm_wide_grid(N, rows)), dim3(512), 0, st, A, W, rows, N, K, e);
    else
        DTK_LAUNCH(name, (gemm_tiled_kernel<T, EPI_SWIGLU>), dim3(gemm_grid(N, rows)), dim3(256), 0, st, A, W, rows, N, K, e);
    return DTK_OK;
}
inline bool vit_swiglu_flags_ok(int flags, const char* who) {
    if (!(flags & (DTK_VIT_GEMM_WIDE_V1 | DTK_VIT_GEMM_WS_V1))) return true;
    dtk_set_error("%s: the SwiGLU feed-forward has no A / B kernel forms: clear %s", who,
                  (flags & DTK_VIT_GEMM_WIDE_V1) ? "DTK_VIT_GEMM_WIDE_V1" : "DTK_VIT_GEMM_WS_V1");
    return false;
}

// One GEMM of a split block (vit_split.h), every SEPI.  (The LDS-DMA form, round 6: fc2 38.3 -> 34.5, qkv 41.4 -> 39.3 ms per step, ViT-L
// 1613 -> 1461 ms.)
//   !path.tiled and N % 128 == 0        gemm_split_dma_kernel<T, SEPI, true>   (wide_v1: <T, SEPI, false>)   gemm_split_dma_grid(N) x 512
//   otherwise                           gemm_split_kernel<T, SEPI>                                           gemm_split_grid(N)     x 256
template <typename T, int SEPI>
int launch_gemm_split(const char* name, const GemmPath& path, const T* Ah, const T* Al, const T* Wh, const T* Wl, long long rows,
                      int N, int K, const SplitEpi<T>& se, hipStream_t st) {
    if (!path.tiled && N % SD_N == 0) {
        const dim3 grid(gemm_split_dma_grid(N, rows));
        if constexpr (SEPI == SEPI_SWIGLU)   // (staged only; the flag is refused for such a model)
            DTK_LAUNCH(name, (gemm_split_dma_kernel<T, SEPI, true>), grid, dim3(512), 0, st, Ah, Al, Wh, Wl, rows, N, K, se);
        else if (path.wide_v1)
            DTK_LAUNCH(name, (gemm_split_dma_kernel<T, SEPI, false>), grid, dim3(512), 0, st, Ah, Al, Wh, Wl, rows, N, K, se);
        else
            DTK_LAUNCH(name, (gemm_split_dma_kernel<T, SEPI, true>), grid, dim3(512), 0, st, Ah, Al, Wh, Wl, rows, N, K, se);
        return DTK_OK;
    }
    DTK_LAUNCH(name, (gemm_split_kernel<T, SEPI>), dim3(gemm_split_grid(N, rows)), dim3(256), 0, st, Ah, Al, Wh, Wl, rows, N, K, se);
    return DTK_OK;
}

template <typename T>
int vit_run(const dtk_vit_model* m, const float* frames, int nframes, int video_h, int video_w, float* tokens_out,
            float* feat_out, float* qkv_out, unsigned char* ws, const VitPlan& p, int ph, int pw, hipStream_t st) {
    const int HW = ph * pw, D = m->D;
    // the feed-forward: GELU MLP (hidden 4 D) or, ViT-g, SwiGLU -- fc1_w is then the PACKED w12 [2 hidden][D] (include/dtk.h) and the
    // GEMM's epilogue writes silu(gate) * value, fc2_w is w3 [D][hidden]; `hid` is sized for 4 D >= hidden
    const bool swiglu = m->ffn == DTK_VIT_FFN_SWIGLU;
    const int HID = m->hidden > 0 ? m->hidden : 4 * D;
    float* x = reinterpret_cast<float*>(ws + p.x);
    auto at = [&](size_t off) { return reinterpret_cast<T*>(ws + off); };
    T *xn = at(p.xn), *q = at(p.q), *k = at(p.k), *vt = at(p.vt), *ao = at(p.ao), *hid = at(p.hid), *delta = at(p.delta);
    T *xn_lo = at(p.xn_lo), *q_lo = at(p.q_lo), *k_lo = at(p.k_lo), *vt_lo = at(p.vt_lo), *ao_lo = at(p.ao_lo), *hid_lo = at(p.hid_lo);
    int* ovf = m->overflow;
    // Saturation of Q / K / V^T and of the MLP hidden (overflow bits 2 / 4): tracked for EVERY value of EVERY frame inside the
    // epilogues of the QKV and fc1 GEMMs (GemmEpi::ovf, round 5: four v_max3 per eight values, no extra pass; rounds 3-4 scanned
    // the first frame of a call only, so a later frame could saturate silently).  DTK_VIT_CHECK_RANGE additionally scans the
    // stored tensors of every block (a pass over 1.3 GB per block and 30 frames): the cross-check of the tests.
    const bool scan_all = ovf && (m->flags & DTK_VIT_CHECK_RANGE);
    int* const epi_ovf = IsF16<T>::value ? ovf : nullptr;
    const int S = p.S, Sp = p.Sp;
    // Q/K/V^T padding rows (s >= S) must be finite zeros: they are read by the last KV tile
    {
        const long long n16 = (long long)((p.ao - p.q) / 16);
        DTK_LAUNCH("vit_zero", zero_kernel, dim3(dtk_cdiv(n16, 256)), dim3(256), 0, st, reinterpret_cast<uint4*>(q), n16);
        if (p.split) {
            const long long m16 = (long long)((p.ao_lo - p.q_lo) / 16);
            DTK_LAUNCH("vit_zero", zero_kernel, dim3(dtk_cdiv(m16, 256)), dim3(256), 0, st, reinterpret_cast<uint4*>(q_lo), m16);
        }
    }
    for (int f0 = 0; f0 < nframes; f0 += p.FB) {
        const int nf = (nframes - f0) < p.FB ? (nframes - f0) : p.FB;
        const long long rows = (long long)nf * S;
        auto scan_range = [&](const T* t, long long n, int bit) -> int {
            const int blocks = (int)(dtk_cdiv(n / 8, 256) < 1024 ? dtk_cdiv(n / 8, 256) : 1024);
            DTK_LAUNCH("vit_range_scan", range_scan_kernel<T>, dim3(blocks), dim3(256), 0, st, t, n / 8, ovf, bit);
            return DTK_OK;
        };
        const bool pe_fits = (size_t)nf * video_h * video_w * 16 <= p.delta - p.hid &&
                             (size_t)D * PE_K * 4 <= p.total - p.delta;
        if (m->patch == PE_P && m->stride == PE_S && pe_fits) {
            // split planes of the normalised frames live in `hid`, the split weights in `delta` (both unused until the
            // first block)
            h4v* fh = reinterpret_cast<h4v*>(hid);
            h4v* fl = fh + (size_t)nf * video_h * video_w;
            half_t* wh = reinterpret_cast<half_t*>(delta);
            half_t* wl = wh + (size_t)D * PE_K;
            const long long npix = (long long)nf * video_h * video_w;
            DTK_LAUNCH("vit_frame_split", frame_split4_kernel, dim3(dtk_cdiv(npix, 256)), dim3(256), 0, st,
                       frames + (size_t)f0 * 3 * video_h * video_w, m->mean_std, fh, fl, video_h, video_w, npix);
            DTK_LAUNCH("vit_frame_split", pack_patch_split_kernel, dim3(dtk_cdiv((long long)D * PE_K, 256)), dim3(256), 0, st,
                       m->patch_w, D, wh, wl);
            const int groups_x = dtk_cdiv(pw, PE_TOK);
            const int units = groups_x * ph * nf, slabs = dtk_cdiv(D, PE_NF);
            DTK_LAUNCH("vit_patch_embed", patch_embed_split_kernel, dim3(8 * dtk_cdiv(units, 8) * slabs), dim3(256), 0, st, fh,
                       fl, wh, wl, m->patch_b, m->pos, m->cls_pos, x, video_h, video_w, ph, pw, D, S, groups_x, units, slabs);
        } else {
            DTK_LAUNCH("vit_patch_embed", patch_embed_kernel, dim3(dtk_cdiv(HW, 64), dtk_cdiv(D, 64), nf), dim3(256), 0, st,
                       frames + (size_t)f0 * 3 * video_h * video_w, m->patch_w, m->patch_b, m->pos, m->cls_pos, m->mean_std,
                       x, video_h, video_w, ph, pw, D, m->patch, m->stride, S);
        }
        // The residual updates of a fast block (LayerScale'd projection / MLP outputs) are written as `delta` and added by the next
        // LayerNorm; which kernel a GEMM runs on: launch_gemm / launch_gemm_split above.
        const GemmPath path = gemm_path(m);
        // DTK_DEV: bits 0-1 skip the weight-stationary kernel's stores; gemm_wide_kernel: 4 no stores, 8 no main loop (pipeline fill +
        // epilogue only), 16 every stage from k = 0 (cache-hot operands)
        const int dbg_ns = DTK_DBG(dtk_dev_flags() >> 16, 0xff);
        bool pending = false;   // `delta` holds a residual update that the next LayerNorm (or the final update) has to apply
        bool ln1_done = false;  // the previous block's fc2 has already written this block's LayerNorm-1 rows to xn (round 6)
        auto tap = [&](int l, bool with_delta) -> int {   // dtk_vit_model.tap_out: the block output of layer l joins the mean
            if (!m->tap_out || !((m->tap_mask >> l) & 1)) return DTK_OK;
            const long long t4 = rows * (D / 4);
            DTK_LAUNCH("vit_tap", tap_kernel<T>, dim3(dtk_cdiv(t4, 256)), dim3(256), 0, st, x, with_delta ? (const T*)delta : (const T*)nullptr,
                       m->tap_out + (size_t)f0 * S * D, m->tap_scale, t4);
            return DTK_OK;
        };
        for (int l = 0; l < m->depth; ++l) {
            const dtk_vit_layer& L = m->layers[l];
            const T* qkv_w = reinterpret_cast<const T*>(L.qkv_w);
            const T* proj_w = reinterpret_cast<const T*>(L.proj_w);
            const T* fc1_w = reinterpret_cast<const T*>(L.fc1_w);
            const T* fc2_w = reinterpret_cast<const T*>(L.fc2_w);
            if (vit_layer_split(L)) {
                // ---- the escalated precision (vit_split.h): every product on hi + lo operands, updates straight into x ----
                const T* qkv_wl = reinterpret_cast<const T*>(L.qkv_w_lo);
                const T* proj_wl = reinterpret_cast<const T*>(L.proj_w_lo);
                const T* fc1_wl = reinterpret_cast<const T*>(L.fc1_w_lo);
                const T* fc2_wl = reinterpret_cast<const T*>(L.fc2_w_lo);
                const float inv_ws = 1.f / (L.w_scale > 0.f ? L.w_scale : 1.f);
                if (launch_layernorm_split<T>(x, pending ? (const T*)delta : (const T*)nullptr, L.ln1_w, L.ln1_b, xn, xn_lo, rows, D, m->ln_eps,
                                              ovf, st)) return DTK_E_HIP;
                pending = false;
                SplitEpi<T> se{};
                if (qkv_out && l == m->depth - 1) {
                    se.bias = L.qkv_b; se.inv_wscale = inv_ws; se.out_f32 = qkv_out + (size_t)f0 * S * 3 * D;
                    if (launch_gemm_split<T, SEPI_F32>("vit_gemm_qkv_facet", path, xn, xn_lo, qkv_w, qkv_wl, rows, 3 * D, D, se, st)) return DTK_E_HIP;
                    se = SplitEpi<T>{};
                }
                se.bias = L.qkv_b; se.inv_wscale = inv_ws; se.q_hi = q; se.q_lo = q_lo; se.k_hi = k; se.k_lo = k_lo; se.vt_hi = vt;
                se.vt_lo = vt_lo; se.S = S; se.Sp = Sp; se.heads = m->heads; se.D = D; se.qscale = 0.125f * 1.4426950408889634f;
                se.ovf = epi_ovf;
                if (launch_gemm_split<T, SEPI_QKV>("vit_gemm_qkv_split", path, xn, xn_lo, qkv_w, qkv_wl, rows, 3 * D, D, se, st)) return DTK_E_HIP;
                const int nqb = dtk_cdiv(Sp, 128);
                DTK_LAUNCH("vit_attention_split", attention_split_kernel<T>, dim3((unsigned)(nf * m->heads * nqb)), dim3(256), 0, st,
                           (const T*)q, (const T*)q_lo, (const T*)k, (const T*)k_lo, (const T*)vt, (const T*)vt_lo, ao, ao_lo, S, Sp,
                           m->heads, nqb);
                se = SplitEpi<T>{};
                se.bias = L.proj_b; se.inv_wscale = inv_ws; se.x = x; se.gamma = L.ls1;
                if (launch_gemm_split<T, SEPI_RESID>("vit_gemm_proj_split", path, ao, ao_lo, proj_w, proj_wl, rows, D, D, se, st)) return DTK_E_HIP;
                if (launch_layernorm_split<T>(x, (const T*)nullptr, L.ln2_w, L.ln2_b, xn, xn_lo, rows, D, m->ln_eps, ovf, st)) return DTK_E_HIP;
                se = SplitEpi<T>{};
                se.bias = L.fc1_b; se.inv_wscale = inv_ws; se.out_hi = hid; se.out_lo = hid_lo; se.ovf = epi_ovf;
                if (swiglu ? launch_gemm_split<T, SEPI_SWIGLU>("vit_gemm_fc1_split", path, xn, xn_lo, fc1_w, fc1_wl, rows, 2 * HID, D, se, st)
                           : launch_gemm_split<T, SEPI_GELU>("vit_gemm_fc1_split", path, xn, xn_lo, fc1_w, fc1_wl, rows, HID, D, se, st)) return DTK_E_HIP;
                se = SplitEpi<T>{};
                se.bias = L.fc2_b; se.inv_wscale = inv_ws; se.x = x; se.gamma = L.ls2;
                if (launch_gemm_split<T, SEPI_RESID>("vit_gemm_fc2_split", path, hid, hid_lo, fc2_w, fc2_wl, rows, D, HID, se, st)) return DTK_E_HIP;
                if (tap(l, false)) return DTK_E_HIP;
                continue;
            }
            GemmEpi<T> e{};
            if (!ln1_done && launch_layernorm<T>(x, pending ? (const T*)delta : (const T*)nullptr, L.ln1_w, L.ln1_b, xn, rows, D, m->ln_eps, ovf, st))
                return DTK_E_HIP;
            ln1_done = false;
            pending = true;
            if (qkv_out && l == m->depth - 1) {  // the qkv hook of the reference (models/extractor.py:107-118), fp32 out
                e.bias = L.qkv_b; e.out_f32 = qkv_out + (size_t)f0 * S * 3 * D;
                if (launch_gemm<T, EPI_F32>("vit_gemm_qkv_facet", path, xn, qkv_w, rows, 3 * D, D, e, st)) return DTK_E_HIP;
                e = GemmEpi<T>{};
            }
            e.bias = L.qkv_b; e.q = q; e.k = k; e.vt = vt; e.S = S; e.Sp = Sp; e.heads = m->heads; e.D = D;
            e.qscale = 0.125f * 1.4426950408889634f; e.no_store = dbg_ns; e.ovf = epi_ovf;
            if (launch_gemm<T, EPI_QKV>("vit_gemm_qkv", path, xn, qkv_w, rows, 3 * D, D, e, st)) return DTK_E_HIP;
            if (scan_all && scan_range(q, (long long)(p.ao - p.q) / 2, 2)) return DTK_E_HIP;
            if (attention_launch(q, k, vt, ao, S, Sp, m->heads, D, nf * m->heads, (m->flags & DTK_VIT_ATTENTION_V4) != 0, st)) return DTK_E_HIP;
            e = GemmEpi<T>{};
            e.bias = L.proj_b; e.delta = delta; e.gamma = L.ls1; e.no_store = dbg_ns;
            // LayerNorm-2 runs inside the projection's epilogue (gemm_ws_ln_kernel: x += update, xn = the normalised rows; the update is
            // not stored) -- `pending` / `ln1_done` speak of fc2's update and LayerNorm-1 only, and stay as they are
            if (path.proj_ln) { e.ln_x = x; e.ln_w = L.ln2_w; e.ln_b = L.ln2_b; e.ln_out = xn; e.ln_eps = m->ln_eps; e.ln_ovf = ovf; }
            if (launch_gemm<T, EPI_DELTA>("vit_gemm_proj", path, ao, proj_w, rows, D, D, e, st)) return DTK_E_HIP;
            if (!path.proj_ln && launch_layernorm<T>(x, (const T*)delta, L.ln2_w, L.ln2_b, xn, rows, D, m->ln_eps, ovf, st)) return DTK_E_HIP;
            e = GemmEpi<T>{};
            e.bias = L.fc1_b; e.out = hid; e.no_store = dbg_ns; e.ovf = epi_ovf;
            if (swiglu ? launch_gemm_swiglu<T>("vit_gemm_fc1", path, xn, fc1_w, rows, 2 * HID, D, e, st)
                       : launch_gemm<T, EPI_GELU>("vit_gemm_fc1", path, xn, fc1_w, rows, HID, D, e, st)) return DTK_E_HIP;
            if (scan_all && scan_range(hid, rows * HID, 4)) return DTK_E_HIP;
            e = GemmEpi<T>{};
            e.bias = L.fc2_b; e.delta = delta; e.gamma = L.ls2; e.no_store = dbg_ns;
            // round 6: the LayerNorm of the next block runs inside fc2's epilogue when that block is a fast one (the split blocks
            // have their own LayerNorm: hi / lo planes); the last block's update goes to the outputs (below)
            if (path.fc2_ln && l + 1 < m->depth && !vit_layer_split(m->layers[l + 1])) {
                const dtk_vit_layer& Ln = m->layers[l + 1];
                e.ln_x = x; e.ln_w = Ln.ln1_w; e.ln_b = Ln.ln1_b; e.ln_out = xn; e.ln_eps = m->ln_eps; e.ln_ovf = ovf;
                pending = false;      // x is up to date ...
                ln1_done = true;      // ... and xn holds the next block's normalised rows
            }
            if (launch_gemm<T, EPI_DELTA>("vit_gemm_fc2", path, hid, fc2_w, rows, D, HID, e, st)) return DTK_E_HIP;
            if (tap(l, pending)) return DTK_E_HIP;
        }
        if (pending && (tokens_out || feat_out)) {
            // the last MLP's residual update, written straight to the outputs (x itself is dead after the last block)
            const long long t4 = rows * (D / 4);
            DTK_LAUNCH("vit_final_update", final_update_kernel<T>, dim3(dtk_cdiv(t4, 256)), dim3(256), 0, st, x, (const T*)delta,
                       tokens_out ? tokens_out + (size_t)f0 * S * D : (float*)nullptr,
                       feat_out ? feat_out + (size_t)f0 * HW * D : (float*)nullptr, S, D, t4, ovf);
        } else {   // depth 0 (embedding + position encoding only) or a split last block: no pending update
            if (pending &&   // (qkv_out only: keep the residual-update check of the last block)
                launch_layernorm<T>(x, (const T*)delta, (const float*)nullptr, (const float*)nullptr, (T*)nullptr, rows, D, m->ln_eps, ovf, st))
                return DTK_E_HIP;
            if (tokens_out)
                DTK_HIP(hipMemcpyAsync(tokens_out + (size_t)f0 * S * D, x, (size_t)rows * D * sizeof(float),
                                       hipMemcpyDeviceToDevice, st));
            if (feat_out) {
                const long long total4 = (long long)nf * HW * (D / 4);
                DTK_LAUNCH("vit_drop_cls", drop_cls_kernel, dim3(dtk_cdiv(total4, 256)), dim3(256), 0, st, x,
                           feat_out + (size_t)f0 * HW * D, S, D, total4);
            }
        }
    }
    return DTK_OK;
}

// ---- one GEMM of a block on its own (dtk_vit_gemm / dtk_vit_gemm_split) ------------------------------------------------------------
// The role names the shape and the epilogue; the kernel is what launch_gemm / launch_gemm_split choose for a model of width D with
// these flags (gemm_path: the dispatch of vit_run, no second table), under the launch names of vit_run.
constexpr int VITG_HIDDEN = 4096;   // upstream vit_giant2: (int(4 * 1536 * 2 / 3) + 7) / 8 * 8
int vit_gemm_check(const dtk_vit_gemm_args* g, const char* who, bool split, int* N, int* K) {
    DTK_REQUIRE(g, "%s: null pointer", who);
    DTK_REQUIRE(g->D == 384 || g->D == 768 || g->D == 1024 || g->D == 1536, "%s: D must be 384, 768 or 1024, or ViT-g's 1536 (got %d)", who, g->D);
    DTK_REQUIRE(g->operand_type == DTK_OPERAND_F16 || g->operand_type == DTK_OPERAND_BF16, "%s: operand_type", who);
    DTK_REQUIRE(g->rows > 0 && g->rows < (1ll << 31), "%s: rows", who);
    DTK_REQUIRE(g->a && g->w && (!split || (g->a_lo && g->w_lo)), "%s: null operand", who);
    const int D = g->D;
    switch (g->role) {
        case DTK_VIT_GEMM_QKV:
            *N = 3 * D; *K = D;
            DTK_REQUIRE(g->q && g->k && g->vt && (!split || (g->q_lo && g->k_lo && g->vt_lo)), "%s: QKV needs q, k and vt", who);
            DTK_REQUIRE(g->S > 0 && g->Sp >= g->S && g->Sp % 64 == 0 && g->rows % g->S == 0,
                        "%s: bad sizes (Sp %% 64 == 0, Sp >= S, rows a multiple of S)", who);
            break;
        case DTK_VIT_GEMM_QKV_FACET:
            *N = 3 * D; *K = D;
            DTK_REQUIRE(g->out_f32, "%s: QKV_FACET needs out_f32", who);
            break;
        case DTK_VIT_GEMM_FC1:
            *N = 4 * D; *K = D;
            DTK_REQUIRE(g->out && (!split || g->out_lo), "%s: FC1 needs out", who);
            break;
        case DTK_VIT_GEMM_PROJ:
        case DTK_VIT_GEMM_FC2:
            *N = D; *K = g->role == DTK_VIT_GEMM_FC2 ? 4 * D : D;
            DTK_REQUIRE(g->gamma && (split ? g->x != nullptr : g->out != nullptr), "%s: PROJ / FC2 need gamma and %s", who, split ? "x" : "out");
            break;
        case DTK_VIT_GEMM_FC1_SWIGLU:
        case DTK_VIT_GEMM_FC2_SWIGLU:
            DTK_REQUIRE(D == 1536, "%s: the SwiGLU roles are ViT-g's, D = 1536 (got %d)", who, D);
            if (!vit_swiglu_flags_ok(g->flags, who)) return DTK_E_INVALID;
            if (g->role == DTK_VIT_GEMM_FC1_SWIGLU) {
                *N = 2 * VITG_HIDDEN; *K = D;
                DTK_REQUIRE(g->out && (!split || g->out_lo), "%s: FC1_SWIGLU needs out", who);
            } else {
                *N = D; *K = VITG_HIDDEN;
                DTK_REQUIRE(g->gamma && (split ? g->x != nullptr : g->out != nullptr), "%s: FC2_SWIGLU needs gamma and %s", who, split ? "x" : "out");
            }
            break;
        default:
            DTK_REQUIRE(false, "%s: unknown role %d", who, g->role);
    }
    return DTK_OK;
}

template <typename T>
int vit_gemm_stage(const dtk_vit_gemm_args* g, int N, int K, hipStream_t st) {
    const GemmPath path = gemm_path(g->D, g->flags);
    const T *A = reinterpret_cast<const T*>(g->a), *W = reinterpret_cast<const T*>(g->w);
    int* const epi_ovf = IsF16<T>::value ? g->ovf : nullptr;
    GemmEpi<T> e{};
    e.bias = g->bias;
    switch (g->role) {
        case DTK_VIT_GEMM_QKV:
            e.q = reinterpret_cast<T*>(g->q); e.k = reinterpret_cast<T*>(g->k); e.vt = reinterpret_cast<T*>(g->vt);
            e.S = g->S; e.Sp = g->Sp; e.heads = g->D / 64; e.D = g->D; e.qscale = 0.125f * 1.4426950408889634f; e.ovf = epi_ovf;
            return launch_gemm<T, EPI_QKV>("vit_gemm_qkv", path, A, W, g->rows, N, K, e, st);
        case DTK_VIT_GEMM_QKV_FACET:
            e.out_f32 = g->out_f32;
            return launch_gemm<T, EPI_F32>("vit_gemm_qkv_facet", path, A, W, g->rows, N, K, e, st);
        case DTK_VIT_GEMM_FC1:
            e.out = reinterpret_cast<T*>(g->out); e.ovf = epi_ovf;
            return launch_gemm<T, EPI_GELU>("vit_gemm_fc1", path, A, W, g->rows, N, K, e, st);
        case DTK_VIT_GEMM_FC1_SWIGLU:
            e.out = reinterpret_cast<T*>(g->out); e.ovf = epi_ovf;
            return launch_gemm_swiglu<T>("vit_gemm_fc1", path, A, W, g->rows, N, K, e, st);
        default:
            e.delta = reinterpret_cast<T*>(g->out); e.gamma = g->gamma;
            if (g->ln_out) {   // the LayerNorm inside fc2's (the next block's) or the projection's (LayerNorm-2) epilogue: where vit_run fuses it, nowhere else
                DTK_REQUIRE(g->role == DTK_VIT_GEMM_PROJ ? path.proj_ln : path.fc2_ln,
                            "dtk_vit_gemm: the fused LayerNorm is fc2's or the projection's at D = 384 without TILED_GEMMS / GEMM_WIDE_V1 / NO_LN_FUSION (the projection's: nor GEMM_WS_V1)");
                DTK_REQUIRE(g->ln_x && g->ln_w && g->ln_b, "dtk_vit_gemm: the fused LayerNorm needs ln_x, ln_w and ln_b");
                e.ln_x = g->ln_x; e.ln_w = g->ln_w; e.ln_b = g->ln_b; e.ln_out = reinterpret_cast<T*>(g->ln_out); e.ln_eps = g->ln_eps;
                e.ln_ovf = g->ovf;
            }
            return launch_gemm<T, EPI_DELTA>(g->role == DTK_VIT_GEMM_PROJ ? "vit_gemm_proj" : "vit_gemm_fc2", path, A, W, g->rows, N, K, e, st);
    }
}

template <typename T>
int vit_gemm_split_stage(const dtk_vit_gemm_args* g, int N, int K, hipStream_t st) {
    const GemmPath path = gemm_path(g->D, g->flags);
    const T *Ah = reinterpret_cast<const T*>(g->a), *Al = reinterpret_cast<const T*>(g->a_lo);
    const T *Wh = reinterpret_cast<const T*>(g->w), *Wl = reinterpret_cast<const T*>(g->w_lo);
    int* const epi_ovf = IsF16<T>::value ? g->ovf : nullptr;
    SplitEpi<T> se{};
    se.bias = g->bias; se.inv_wscale = 1.f / (g->w_scale > 0.f ? g->w_scale : 1.f);
    switch (g->role) {
        case DTK_VIT_GEMM_QKV:
            se.q_hi = reinterpret_cast<T*>(g->q); se.q_lo = reinterpret_cast<T*>(g->q_lo); se.k_hi = reinterpret_cast<T*>(g->k);
            se.k_lo = reinterpret_cast<T*>(g->k_lo); se.vt_hi = reinterpret_cast<T*>(g->vt); se.vt_lo = reinterpret_cast<T*>(g->vt_lo);
            se.S = g->S; se.Sp = g->Sp; se.heads = g->D / 64; se.D = g->D; se.qscale = 0.125f * 1.4426950408889634f; se.ovf = epi_ovf;
            return launch_gemm_split<T, SEPI_QKV>("vit_gemm_qkv_split", path, Ah, Al, Wh, Wl, g->rows, N, K, se, st);
        case DTK_VIT_GEMM_QKV_FACET:
            se.out_f32 = g->out_f32;
            return launch_gemm_split<T, SEPI_F32>("vit_gemm_qkv_facet", path, Ah, Al, Wh, Wl, g->rows, N, K, se, st);
        case DTK_VIT_GEMM_FC1:
            se.out_hi = reinterpret_cast<T*>(g->out); se.out_lo = reinterpret_cast<T*>(g->out_lo); se.ovf = epi_ovf;
            return launch_gemm_split<T, SEPI_GELU>("vit_gemm_fc1_split", path, Ah, Al, Wh, Wl, g->rows, N, K, se, st);
        case DTK_VIT_GEMM_FC1_SWIGLU:
            se.out_hi = reinterpret_cast<T*>(g->out); se.out_lo = reinterpret_cast<T*>(g->out_lo); se.ovf = epi_ovf;
            return launch_gemm_split<T, SEPI_SWIGLU>("vit_gemm_fc1_split", path, Ah, Al, Wh, Wl, g->rows, N, K, se, st);
        default:
            se.x = g->x; se.gamma = g->gamma;
            return launch_gemm_split<T, SEPI_RESID>(g->role == DTK_VIT_GEMM_PROJ ? "vit_gemm_proj_split" : "vit_gemm_fc2_split", path, Ah, Al,
                                                    Wh, Wl, g->rows, N, K, se, st);
    }
}

// every DTK_VIT_* bit of dtk_vit_model.flags that include/dtk.h defines (bit 8 is retired and not reused)
constexpr int VIT_KNOWN_FLAGS = DTK_VIT_TILED_GEMMS | DTK_VIT_BF16 | DTK_VIT_CHECK_RANGE | DTK_VIT_GEMM_WS_V1 | DTK_VIT_ATTENTION_V4 |
                                DTK_VIT_GEMM_WIDE_V1 | DTK_VIT_NO_LN_FUSION;

}  // namespace

extern "C" size_t dtk_vit_workspace_bytes(const dtk_vit_model* m, int video_h, int video_w, int frames) {
    if (!m || frames <= 0) return 0;
    const int ph = 1 + (video_h - m->patch) / m->stride, pw = 1 + (video_w - m->patch) / m->stride;
    return vit_plan(m, ph, pw, frames).total;
}

extern "C" int dtk_vit_forward(const dtk_vit_model* m, const float* frames, int nframes, int video_h, int video_w,
                               float* tokens_out, float* feat_out, float* qkv_out, void* workspace,
                               size_t workspace_bytes, void* stream) {
    DTK_REQUIRE(m && frames && workspace && (tokens_out || feat_out || qkv_out || m->tap_out), "dtk_vit_forward: null pointer");
    DTK_REQUIRE(!(m->flags & ~VIT_KNOWN_FLAGS), "dtk_vit_forward: unknown flag bits 0x%x (bit 8 selected a kernel that left the library)",
                (unsigned)(m->flags & ~VIT_KNOWN_FLAGS));
    DTK_REQUIRE(!qkv_out || m->depth > 0, "dtk_vit_forward: qkv_out needs at least one block");
    DTK_REQUIRE(m->D > 0 && m->heads > 0 && m->D == m->heads * 64, "dtk_vit_forward: d_head must be 64 (D=%d heads=%d)",
                m->D, m->heads);
    DTK_REQUIRE(m->D % 32 == 0 && m->depth >= 0 && m->layers, "dtk_vit_forward: bad model");
    DTK_REQUIRE(m->D <= VIT_MAX_D, "dtk_vit_forward: D = %d: the LayerNorm kernels hold rows of at most %d channels", m->D, VIT_MAX_D);
    if (m->ffn == DTK_VIT_FFN_SWIGLU) {
        DTK_REQUIRE(m->D == 1536 && m->hidden == VITG_HIDDEN, "dtk_vit_forward: the SwiGLU feed-forward is ViT-g's: D = 1536, hidden = %d (got D = %d, hidden = %d)",
                    VITG_HIDDEN, m->D, m->hidden);
        if (!vit_swiglu_flags_ok(m->flags, "dtk_vit_forward")) return DTK_E_INVALID;
    } else {
        DTK_REQUIRE(m->ffn == DTK_VIT_FFN_GELU, "dtk_vit_forward: unknown ffn %d", m->ffn);
        DTK_REQUIRE(m->hidden == 0 || m->hidden == 4 * m->D, "dtk_vit_forward: a GELU MLP has hidden = 4 D (got %d)", m->hidden);
    }
    DTK_REQUIRE(video_h >= m->patch && video_w >= m->patch, "dtk_vit_forward: frame smaller than a patch");
    const int ph = 1 + (video_h - m->patch) / m->stride, pw = 1 + (video_w - m->patch) / m->stride;
    const VitPlan p = vit_plan(m, ph, pw, nframes);
    if (workspace_bytes < p.total) {
        dtk_set_error("dtk_vit_forward: workspace %zu B < required %zu B", workspace_bytes, p.total);
        return DTK_E_WORKSPACE;
    }
    hipStream_t st = dtk_stream(stream);
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    if (m->flags & DTK_VIT_BF16)
        return vit_run<__bf16>(m, frames, nframes, video_h, video_w, tokens_out, feat_out, qkv_out, ws, p, ph, pw, st);
    return vit_run<_Float16>(m, frames, nframes, video_h, video_w, tokens_out, feat_out, qkv_out, ws, p, ph, pw, st);
}

// The attention stage on its own (tests drive its guard / safe-pass logic with crafted operands; layouts as inside
// dtk_vit_forward).
extern "C" int dtk_vit_attention(const void* q, const void* k, const void* vt, void* out, int frames, int heads, int S,
                                 int Sp, int operand_type, void* stream) {
    DTK_REQUIRE(q && k && vt && out, "dtk_vit_attention: null pointer");
    DTK_REQUIRE(frames > 0 && heads > 0 && S > 0 && Sp >= S && Sp % 64 == 0, "dtk_vit_attention: bad sizes (Sp %% 64 == 0, Sp >= S)");
    const bool v4 = (operand_type & DTK_OPERAND_ATTENTION_V4) != 0;
    operand_type &= ~DTK_OPERAND_ATTENTION_V4;   // any other bit (the retired kernel selections among them) is refused below
    DTK_REQUIRE(operand_type == DTK_OPERAND_F16 || operand_type == DTK_OPERAND_BF16, "dtk_vit_attention: operand_type");
    if (operand_type == DTK_OPERAND_BF16)
        return attention_launch(reinterpret_cast<const __bf16*>(q), reinterpret_cast<const __bf16*>(k),
                                reinterpret_cast<const __bf16*>(vt), reinterpret_cast<__bf16*>(out), S, Sp, heads, heads * 64,
                                frames * heads, v4, dtk_stream(stream));
    return attention_launch(reinterpret_cast<const _Float16*>(q), reinterpret_cast<const _Float16*>(k),
                            reinterpret_cast<const _Float16*>(vt), reinterpret_cast<_Float16*>(out), S, Sp, heads, heads * 64,
                            frames * heads, v4, dtk_stream(stream));
}

// The same stage on split operands (vit_split.h: the escalated precision): hi / lo planes of every operand and of the output.
extern "C" int dtk_vit_attention_split(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* vt_hi,
                                       const void* vt_lo, void* out_hi, void* out_lo, int frames, int heads, int S, int Sp,
                                       int operand_type, void* stream) {
    DTK_REQUIRE(q_hi && q_lo && k_hi && k_lo && vt_hi && vt_lo && out_hi && out_lo, "dtk_vit_attention_split: null pointer");
    DTK_REQUIRE(frames > 0 && heads > 0 && S > 0 && Sp >= S && Sp % 64 == 0, "dtk_vit_attention_split: bad sizes (Sp %% 64 == 0, Sp >= S)");
    DTK_REQUIRE(operand_type == DTK_OPERAND_F16 || operand_type == DTK_OPERAND_BF16, "dtk_vit_attention_split: operand_type");
    hipStream_t st = dtk_stream(stream);
    const int nqb = dtk_cdiv(Sp, 128);
    const unsigned grid = (unsigned)(frames * heads * nqb);
    if (operand_type == DTK_OPERAND_BF16) {
        typedef __bf16 T;
        DTK_LAUNCH("vit_attention_split", attention_split_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)q_hi, (const T*)q_lo,
                   (const T*)k_hi, (const T*)k_lo, (const T*)vt_hi, (const T*)vt_lo, (T*)out_hi, (T*)out_lo, S, Sp, heads, nqb);
    } else {
        typedef _Float16 T;
        DTK_LAUNCH("vit_attention_split", attention_split_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)q_hi, (const T*)q_lo,
                   (const T*)k_hi, (const T*)k_lo, (const T*)vt_hi, (const T*)vt_lo, (T*)out_hi, (T*)out_lo, S, Sp, heads, nqb);
    }
    return DTK_OK;
}


// One GEMM of a block on its own (tests compare every kernel form with float64 on the operands it read; layouts and dispatch as
// inside dtk_vit_forward).
extern "C" int dtk_vit_gemm(const dtk_vit_gemm_args* g, void* stream) {
    int N = 0, K = 0;
    if (const int rc = vit_gemm_check(g, "dtk_vit_gemm", false, &N, &K)) return rc;
    if (g->operand_type == DTK_OPERAND_BF16) return vit_gemm_stage<__bf16>(g, N, K, dtk_stream(stream));
    return vit_gemm_stage<_Float16>(g, N, K, dtk_stream(stream));
}

// The same stage on split operands (vit_split.h): hi / lo planes of A, of w_scale * W and of the 16-bit outputs; the residual roles
// add their update to the fp32 stream x.
extern "C" int dtk_vit_gemm_split(const dtk_vit_gemm_args* g, void* stream) {
    int N = 0, K = 0;
    if (const int rc = vit_gemm_check(g, "dtk_vit_gemm_split", true, &N, &K)) return rc;
    DTK_REQUIRE(!g->ln_out, "dtk_vit_gemm_split: the split blocks have their own LayerNorm");
    if (g->operand_type == DTK_OPERAND_BF16) return vit_gemm_split_stage<__bf16>(g, N, K, dtk_stream(stream));
    return vit_gemm_split_stage<_Float16>(g, N, K, dtk_stream(stream));
}
