// vit_gemm_common.h -- what the GEMM kernels of the ViT encoder (vit_gemm_tiled / ws / wide.h, vit_split.h) and vit.hip share: the
// operand-type plumbing, the epilogue descriptor GemmEpi and its tile epilogues, the LDS swizzle, the packed GELU and the issue
// of one pipeline stage by descriptor LDS-DMA.  Everything lives in the anonymous namespace of the one translation unit, vit.hip.
#pragma once
#include "common.h"

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef _Float16 half_t;
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4v __attribute__((ext_vector_type(4)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));

// operand-type plumbing of the templated kernels below
template <typename T> struct Vec {
    typedef T t8 __attribute__((ext_vector_type(8)));
    typedef T t4 __attribute__((ext_vector_type(4)));
    typedef T t2 __attribute__((ext_vector_type(2)));
};
template <typename T> struct IsF16 { static constexpr bool value = false; };
template <> struct IsF16<_Float16> { static constexpr bool value = true; };
__device__ __forceinline__ f4 mfma16(h8 a, h8 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f4 mfma16(bf8 a, bf8 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f16v mfma32(h8 a, h8 b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f16v mfma32(bf8 a, bf8 b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
template <typename T> __device__ __forceinline__ void operand_mode() {
    if (IsF16<T>::value) dtk_fp16_saturate_mode();  // overflowing fp16 results clamp to +-65504 instead of +-inf
}

// ---------------------------------------------------------------------------------------------------------------
// bf16 GEMM  C[M][N] = A[M][K] . Wt[N][K]^T (+bias) with fused epilogues
// ---------------------------------------------------------------------------------------------------------------
constexpr int GM = 128, GN = 128, GK = 32;
enum { EPI_QKV = 0, EPI_GELU = 1, EPI_DELTA = 2, EPI_F32 = 3, EPI_SWIGLU = 4 };

template <typename T>
struct GemmEpi {
    const float* bias;   // [N]
    // EPI_QKV
    T* q;           // [F][heads][Sp][64]
    T* k;           // [F][heads][Sp][64]
    T* vt;          // [F][heads][64][Sp]
    int S, Sp, heads, D;
    float qscale;
    // EPI_GELU; EPI_SWIGLU: [M][N / 2] (the packed w12 rows, see swiglu_col)
    T* out;         // [M][N]
    // EPI_DELTA
    int no_store;        // DTK_DEV builds: DTK_DEBUG >> 16 -- 1 | 2: skip the stores of the weight-stationary kernel; 4 .. 16: the wide kernels;
                         // 32 / 64 / 128: gemm_ws_kernel's clean ablations and its form before the hand-cut step (vit_gemm_ws.h)
    T* delta;       // [M][N] bf16: gamma * (A W^T + bias), added to the fp32 residual stream by the next LayerNorm
    const float* gamma;  // [N] LayerScale
    // EPI_F32 (tiled kernel only)
    float* out_f32;      // [M][N] fp32: A W^T + bias (the qkv facet output)
    // fp16 range (round 5): EPI_QKV / EPI_GELU kernels OR bit 2 / 4 into *ovf when a value they store reaches the fp16 limit --
    // every frame, inside the epilogue (no extra pass); NULL = not tracked (bf16 operands)
    int* ovf;
    // gemm_wide_delta_kernel<T, true, true> (round 6): the LayerNorm of the NEXT block inside fc2's epilogue -- x += delta where the
    // delta tile is staged, statistics and the 16-bit normalised row from the same registers (the arithmetic of layernorm_kernel)
    float* ln_x;             // [M][N] the fp32 residual stream
    const float *ln_w, *ln_b;
    T* ln_out;               // [M][N]
    float ln_eps;
    int* ln_ovf;             // overflow word: bit 1 = a saturated residual update (fp16 operands)
};

// running |max| of the values an epilogue stores (the saturation test of the fp16 range, see GemmEpi::ovf): two values per
// v_max3_f32 with |.| source modifiers.  NaN passes through fmaxf unnoticed: a non-finite activation surfaces in the next
// residual update, which the LayerNorm kernel checks for every token (overflow bit 1).
__device__ __forceinline__ float amax2(float m, float a, float b) { return fmaxf(fmaxf(m, fabsf(a)), fabsf(b)); }
template <typename T, int EPI>
__device__ __forceinline__ void amax_report(float amax, int* ovf) {
    if (IsF16<T>::value && (EPI == EPI_QKV || EPI == EPI_GELU || EPI == EPI_SWIGLU) && ovf) {
        // (65488 = the midpoint below 65504: an fp32 value from there on is STORED as 65504, which the explicit scan of the tensor
        //  -- DTK_VIT_CHECK_RANGE -- reports)
        if (__any(amax >= 65488.f) && (threadIdx.x & 63) == 0) atomicOr(ovf, EPI == EPI_QKV ? 2 : 4);
    }
}

// SwiGLU feed-forward of ViT-g (upstream SwiGLUFFNFused): hidden[j] = silu(pre[j]) * pre[H + j], pre = A w12^T + b12, H = 4096.  The
// rows of w12 / b12 are PACKED on the host (include/dtk.h, dtk_vit_model.ffn) so that every aligned group of 64 packed columns is 32 gate
// columns followed by their 32 value columns: in all four GEMM forms a wave owns 64 consecutive columns as four 16-wide MFMA fragments
// ni = 0 .. 3, so gate (ni = 0, 1) and value (ni + 2) of a pair are accumulators of the SAME lane and the product costs no second pass.
// Packed column n of a gate fragment -> hidden column:
__device__ __forceinline__ int swiglu_col(int n) { return ((n >> 6) << 5) + (n & 31); }
// silu(v) = v / (1 + exp(-v)) in fp32 from the accumulator: exp through v_exp_f32 (1 ulp) on -v log2(e), the quotient through v_rcp_f32
// (1 ulp).  Finite for every finite v: exp(-v) = +inf for v < -88.8 gives v * 0 = -0, exp(-v) = 0 for large v gives v.
// SILU_ERR: |silu~(v) - silu(v)| <= 4e-7 * max(1, |v|)  (five roundings of <= 1 ulp on a result of magnitude <= |v|, and the argument's
// rounding |v| 2^-24 acting on exp only where silu is small; an fp32 emulation measures 1.8e-7 over [-100, 100] and at +-1e4:
// tests/test_vitg_reference.py).
__device__ __forceinline__ float silu_f32(float v) {
    const float e = __builtin_amdgcn_exp2f(v * -1.4426950408889634f);
    return v * __builtin_amdgcn_rcpf(1.f + e);
}
// one pair: what is stored (before the rounding to T), and its |.| into the running maximum of the fp16 range check
__device__ __forceinline__ float swiglu_pair(float gate, float value, float& amax) {
    const float h = silu_f32(gate) * value;
    amax = fmaxf(amax, fabsf(h));
    return h;
}

// LDS image of an operand tile: row-major, four 16-byte pieces per row, piece p of row r in slot p ^ gswz_f(r)
__device__ __forceinline__ int gswz_f(int row) { return (0x1230 >> (((row >> 2) & 3) * 4)) & 3; }  // {0,3,2,1}: conflict-free ds_read_b128 fragments
__device__ __forceinline__ int gswz(int row, int piece) { return row * 4 + (piece ^ gswz_f(row)); }
// 16 bytes of a staged output row whose pitch is only 8-byte aligned: two ds_read_b64
__device__ __forceinline__ uint4 staged16(const unsigned char* sp) {
    const uint2 lo = *reinterpret_cast<const uint2*>(sp), hi = *reinterpret_cast<const uint2*>(sp + 8);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

// Epilogue of one 16x16 D tile: lane (fg, fj) holds rows mb .. mb+3 of column n (a[r]).  Shared by the tiled kernels.
template <typename T, int EPI>
__device__ __forceinline__ void gemm_store_tile(const f4& a, long long mb, int n, float bias, long long M, int N,
                                                const GemmEpi<T>& e, float& amax) {
    if (IsF16<T>::value && (EPI == EPI_QKV || EPI == EPI_GELU)) {   // rows past M hold the repeated last row: harmless
        const float sc = (EPI == EPI_QKV && n < e.D) ? e.qscale : 1.f;
        // what is STORED: Q already scaled; for the MLP hidden GELU(v) -- v for large positive v, ~0 for negative ones (ADVICE r5:
        // the pre-activation's |v| flagged a harmless v <= -65504): the positive part
        if (EPI == EPI_GELU) amax = fmaxf(fmaxf(fmaxf(amax, a[0] + bias), fmaxf(a[1] + bias, a[2] + bias)), a[3] + bias);
        else amax = amax2(amax2(amax, (a[0] + bias) * sc, (a[1] + bias) * sc), (a[2] + bias) * sc, (a[3] + bias) * sc);
    }
    if (EPI == EPI_QKV) {
        const int which = n / e.D, rem = n - which * e.D;
        const int head = rem >> 6, dh = rem & 63;
        const int frame = (int)(mb / e.S);  // the 4 rows of a fragment may straddle two frames: handle per row
        (void)frame;
        if (which == 2) {
            // V transposed: 4 consecutive tokens -> 8 contiguous bytes when they stay inside one frame
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long m = mb + r;
                if (m < M) {
                    const int f = (int)(m / e.S), s = (int)(m - (long long)f * e.S);
                    e.vt[(((size_t)f * e.heads + head) * 64 + dh) * e.Sp + s] = (T)(a[r] + bias);
                }
            }
        } else {
            T* dst = which == 0 ? e.q : e.k;
            const float sc = which == 0 ? e.qscale : 1.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long m = mb + r;
                if (m < M) {
                    const int f = (int)(m / e.S), s = (int)(m - (long long)f * e.S);
                    dst[(((size_t)f * e.heads + head) * e.Sp + s) * 64 + dh] = (T)((a[r] + bias) * sc);
                }
            }
        }
    } else if (EPI == EPI_GELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long m = mb + r;
            if (m < M) {
                const float v = a[r] + bias;
                e.out[m * N + n] = (T)(0.5f * v * (1.f + erff(v * 0.70710678118654752f)));
            }
        }
    } else if (EPI == EPI_F32) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long m = mb + r;
            if (m < M) e.out_f32[m * N + n] = a[r] + bias;
        }
    } else {
        const float gm = e.gamma[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long m = mb + r;
            if (m < M) e.delta[m * N + n] = (T)(gm * (a[r] + bias));
        }
    }
}

// EPI_SWIGLU on the tiled kernel: gate tile `a` (packed column n, bias bg) and value tile `b` (packed column n + 32, bias bv) of rows
// mb .. mb + 3 -> out[m][swiglu_col(n)], N = the PACKED width
template <typename T>
__device__ __forceinline__ void gemm_store_tile_swiglu(const f4& a, const f4& b, long long mb, int n, float bg, float bv, long long M,
                                                       int N, const GemmEpi<T>& e, float& amax) {
    const int hc = swiglu_col(n), NH = N >> 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float h = swiglu_pair(a[r] + bg, b[r] + bv, amax);   // rows past M hold the repeated last row: harmless
        if (mb + r < M) e.out[(mb + r) * NH + hc] = (T)h;
    }
}

// One wave's share of a pipeline stage of the wide GEMMs by DESCRIPTOR LDS-DMA (round 6; common.h dtk_buffer_lds16: three issue
// slots per request where the global_load_lds form, dtk_glds16, costs ~13 -- 64-bit address arithmetic on the VALU, m0 saved and
// restored).
// Request i of wave w lands at stage + (w REQ + i) KB: the stages of gemm_wide_delta / gemm_wide / gemm_split_dma are laid out so.
// srd[i] = descriptor over the first row of the request's operand tile, voff[i] = the lane's constant byte offset in it (row, swizzled
// piece), soff = the k-step's byte offset.  A kernel that calls this must not use dtk_glds16 (m0: tests/test_abi.py::test_m0_users).
template <int REQ, int I = 0>
__device__ __forceinline__ void wd_issue(const dtk_u4 (&srd)[REQ], const unsigned (&voff)[REQ], unsigned soff, unsigned lds_dst) {
    dtk_buffer_lds16<I * 1024>(srd[I], soff, voff[I], lds_dst);
    if constexpr (I + 1 < REQ) wd_issue<REQ, I + 1>(srd, voff, soff, lds_dst);
}

// GELU(x) = x Phi(x) with erf(s / sqrt 2) ~ s P(s^2) on |s| <= 4.25 (odd minimax polynomial, 9 coefficients, |err| < 2e-5;
// |GELU error| < 6e-5 for x >= -12, far below the bf16 rounding of the result; below that the clamp leaves x / 2 * (1 + erf~(-4.25 / sqrt 2)),
// about 4.8e-6 |x| where GELU is 0 -- measured by tests/test_gpu_vit_gemm.py); two values per packed fp32 instruction
__device__ __forceinline__ f2 gelu2(f2 x) {
    const f2 c = {4.25f, 4.25f};
    const f2 sx = __builtin_elementwise_min(__builtin_elementwise_max(x, -c), c);
    const f2 u = sx * sx;
    f2 p = {1.112979639e-10f, 1.112979639e-10f};
    p = __builtin_elementwise_fma(p, u, f2{-1.065557687e-08f, -1.065557687e-08f});
    p = __builtin_elementwise_fma(p, u, f2{4.510875158e-07f, 4.510875158e-07f});
    p = __builtin_elementwise_fma(p, u, f2{-1.125288873e-05f, -1.125288873e-05f});
    p = __builtin_elementwise_fma(p, u, f2{1.868377149e-04f, 1.868377149e-04f});
    p = __builtin_elementwise_fma(p, u, f2{-2.217123518e-03f, -2.217123518e-03f});
    p = __builtin_elementwise_fma(p, u, f2{1.963194646e-02f, 1.963194646e-02f});
    p = __builtin_elementwise_fma(p, u, f2{-1.326889843e-01f, -1.326889843e-01f});
    p = __builtin_elementwise_fma(p, u, f2{7.978046536e-01f, 7.978046536e-01f});
    const f2 one = {1.f, 1.f};
    const f2 e = __builtin_elementwise_min(__builtin_elementwise_max(sx * p, -one), one);
    const f2 hx = x * f2{0.5f, 0.5f};
    return __builtin_elementwise_fma(hx, e, hx);
}

// Epilogue of one TRANSPOSED 16x16 D tile (gemm_wide_kernel, round 5: its MFMAs run as (W tile) x (token tile)^T, so a lane
// holds four CONSECUTIVE output features nb .. nb+3 of ONE token m): one 8-byte store per tile and lane where the layout keeps
// features contiguous (GELU hidden, residual update, Q, K) instead of four 2-byte stores -- 32 store instructions per lane and
// 256 x 256 tile instead of 128 (the wide models' fc1 / qkv ran at 0.55 / 0.60 PF against fc2's 1.06 on the same main loop:
// profiles/r04_bench_width1024.json).  V^T keeps tokens contiguous, so its four features go out as 2-byte stores of 16 lanes = 32 B.
template <typename T, int EPI>
__device__ __forceinline__ void gemm_store_tile_t(const f4& a, long long m, int nb, long long M, int N, const GemmEpi<T>& e,
                                                  float& amax) {
    typedef typename Vec<T>::t4 T4;
    const float4 b4 = e.bias ? *reinterpret_cast<const float4*>(e.bias + nb) : make_float4(0.f, 0.f, 0.f, 0.f);
    float v[4] = {a[0] + b4.x, a[1] + b4.y, a[2] + b4.z, a[3] + b4.w};
    if (EPI == EPI_QKV) {
        const int which = nb / e.D, rem = nb - which * e.D;
        const int head = rem >> 6, dh = rem & 63;
        const float sc = which == 0 ? e.qscale : 1.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] *= sc;
        if (IsF16<T>::value) amax = amax2(amax2(amax, v[0], v[1]), v[2], v[3]);
        if (m >= M || DTK_DBG(e.no_store, 4)) return;
        const int f = (int)(m / e.S), sp = (int)(m - (long long)f * e.S);
        if (which == 2) {
            T* vp = e.vt + (((size_t)f * e.heads + head) * 64 + dh) * e.Sp + sp;
#pragma unroll
            for (int r = 0; r < 4; ++r) vp[(size_t)r * e.Sp] = (T)v[r];
        } else {
            T* dst = (which == 0 ? e.q : e.k) + (((size_t)f * e.heads + head) * e.Sp + sp) * 64 + dh;
            *reinterpret_cast<T4*>(dst) = T4{(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
        }
    } else if (EPI == EPI_GELU) {
        if (IsF16<T>::value) amax = fmaxf(fmaxf(fmaxf(amax, v[0]), fmaxf(v[1], v[2])), v[3]);   // GELU(v) = v where it is large: the positive part
        if (m >= M || DTK_DBG(e.no_store, 4)) return;
        // (the packed polynomial GELU of the weight-stationary kernels: |error| < 6e-5, below the 16-bit rounding of the result;
        //  libm's erff costs ~10 x the instructions, and this epilogue runs for 4096 features of every token in fc1)
        const f2 g0 = gelu2(f2{v[0], v[1]}), g1 = gelu2(f2{v[2], v[3]});
        *reinterpret_cast<T4*>(e.out + m * N + nb) = T4{(T)g0[0], (T)g0[1], (T)g1[0], (T)g1[1]};
    } else {   // EPI_DELTA
        if (m >= M || DTK_DBG(e.no_store, 4)) return;
        const float4 g4 = *reinterpret_cast<const float4*>(e.gamma + nb);
        *reinterpret_cast<T4*>(e.delta + m * N + nb) = T4{(T)(g4.x * v[0]), (T)(g4.y * v[1]), (T)(g4.z * v[2]), (T)(g4.w * v[3])};
    }
}

// The same tile as a VALUE (EPI_GELU / EPI_DELTA; round 6: gemm_wide_kernel stages its output tile in LDS and writes whole rows)
template <typename T, int EPI>
__device__ __forceinline__ typename Vec<T>::t4 gemm_value_tile_t(const f4& a, const float4& b4, const float4& g4, float& amax) {
    typedef typename Vec<T>::t4 T4;
    const float v[4] = {a[0] + b4.x, a[1] + b4.y, a[2] + b4.z, a[3] + b4.w};
    if (EPI == EPI_GELU) {
        if (IsF16<T>::value) amax = fmaxf(fmaxf(fmaxf(amax, v[0]), fmaxf(v[1], v[2])), v[3]);
        const f2 g0 = gelu2(f2{v[0], v[1]}), g1 = gelu2(f2{v[2], v[3]});
        return T4{(T)g0[0], (T)g0[1], (T)g1[0], (T)g1[1]};
    }
    return T4{(T)(g4.x * v[0]), (T)(g4.y * v[1]), (T)(g4.z * v[2]), (T)(g4.w * v[3])};
}

}  // namespace
