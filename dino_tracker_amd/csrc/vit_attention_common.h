// vit_attention_common.h -- what the flash-attention kernels for d_head = 64 (vit_attention4.h, vit_attention6.h) share: the
// operand type, the K / V^T tile layout, the fp16 range guards, the safe pass, the grid and the AGPR helpers.
//
// fp16 is the default operand type of the library since round 3: the same MFMA rate as bf16 with 8x less operand rounding (round
// 2's end-to-end error from the VIDEO, p99 1.4e-3 px, was the bf16 operands of P1).  fp16's narrow exponent range is what the
// guards below are sized for.
//
// THE GUARD ARITHMETIC (optimistic exponentials; both kernels use it unchanged since round 2).  With d_head = 64 the softmax
// costs as many VALU cycles as the tile costs MFMA cycles, and a third of them only maintain the running maximum.  Any reference
// m gives the same softmax as long as 2^(s - m) stays inside the range in which P keeps its precision: bf16 has fp32's exponent
// range; fp16 ends at 65504 above and has full precision down to 2^-14 only.
//   * The reference is ESTIMATED ONCE per query, before the key loop: the maximum of its scores against the first 64 keys (which
//     hold the CLS token and, for DINOv2 with registers, the register tokens right behind it) and against the 32 keys of its own
//     query tile (which hold its own key: the self score is the usual row maximum of a trained ViT; a trained register model's
//     large-norm registers are among the first 64 keys).  That is a lower bound of the row maximum, hence p_max >= 1.  The
//     kernels feed -m to the scores through the C operand of the first MFMA of a score block, so subtracting it costs no VALU work.
//   * In the loop only a guard on the tile's row sum runs, one compare per tile: not (a lane's 32-key part < Operand::RESC_T),
//     which also catches inf / NaN.  Nothing has overflowed yet while the part stays below Operand::POISON_T (fp16: RESC_T = 2^9,
//     POISON_T = 2^15, so every p < 65504; bf16: 2^40 / 2^120).
//   * The power-of-two rescale: after the tile's PV product the wave moves the reference up by k = floor(log2(tile sum)), i.e.
//     scales l and O by the exact power of two 2^-k (scores already computed against the old reference move by -k with it).
//     The reference therefore never exceeds the row maximum by more than 6 binades (k <= log2(64 p_max)), so p_max >= 2^-6 and
//     the entries that matter at 11 bits are normal numbers.
//   * A part beyond POISON_T in ONE step (fp16: a score 15 binades = 10 nats above everything the row has seen; bf16: 120
//     binades) poisons the row sum (NaN) instead.  A wave that finds a poisoned or a tiny (< Operand::LOW_T) sum at the end
//     redoes its queries in safe_pass below: running maximum per tile, operands straight from global memory, no barriers.
// tests/test_gpu_p1.py::test_attention_guards_and_safe_pass forces all of these events on both kernels.
#pragma once
#include <type_traits>
#include "common.h"

namespace attn {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f16v __attribute__((ext_vector_type(16)));

// operand type T of Q / K / V^T / P / O: _Float16 or __bf16
template <typename T>
struct Operand {
    typedef T v8 __attribute__((ext_vector_type(8)));
    typedef T v4 __attribute__((ext_vector_type(4)));
    typedef T v2 __attribute__((ext_vector_type(2)));
    static constexpr bool F16 = std::is_same<T, _Float16>::value;
    static __device__ __forceinline__ f16v mfma(v8 a, v8 b, f16v c) {
        if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
        else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    // guard thresholds (file comment) on a lane's part (32 keys) of a tile's row sum: at RESC_T the reference moves up after the tile;
    // at POISON_T a P entry may have left the operand type's range (fp16: 65504), the row is redone by the safe pass
    static constexpr float RESC_T = F16 ? 0x1p9f : 0x1p40f;
    static constexpr float POISON_T = F16 ? 0x1p15f : 0x1p120f;
    static constexpr float LOW_T = F16 ? 0x1p-7f : 0x1p-100f;  // a final row sum below this has lost P's precision (fp16 subnormals)
};

constexpr int TILE_KEYS = 64;
constexpr int TILE_BYTES = 2 * TILE_KEYS * 64 * 2;  // K tile (64 keys x 64 d) + V^T tile (64 d x 64 keys), bf16
constexpr int A4_NB = 4;        // LDS ring of attention4 / 6 (buffers of TILE_BYTES)
constexpr int A4_AHEAD = 3;     // tiles requested ahead of the one whose V^T part is being read

// 1-D grid of 8 * ceil(FH / 8) * QB workgroups, QB = ceil(S / queries per workgroup).  Workgroup b runs on XCD b % 8; a kernel maps
// it to (fh, query block) so that all query blocks of one (frame, head) share an XCD and its L2.
inline unsigned attention_grid(int FH, int S, int queries, int* qb_out) {
    const int QB = (S + queries - 1) / queries;
    *qb_out = QB;
    return (unsigned)(((FH + 7) / 8) * 8 * QB);
}

// Combine a per-lane value with the one of lane ^ 32 (the two halves of a wave hold the two key halves of a query) without
// an LDS round trip: v_permlane32_swap exchanges the upper half of its first operand with the lower half of its second.
// NB the two results are copied into scalars BEFORE the bit cast: `__builtin_bit_cast(float, sw[1])` applied to the vector
// element directly reads element 0 under hipcc / ROCm 7.2 (seen in the ISA: both uses came from the first register), which
// silently drops the other half.
__device__ __forceinline__ void halves(float x, float& lo_all, float& hi_all) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    const unsigned r0 = sw[0], r1 = sw[1];
    lo_all = __uint_as_float(r0);  // the value held by the lower-half lane of the pair (lanes 0..31), in both lanes
    hi_all = __uint_as_float(r1);  // the value held by the upper-half lane
}

// Safe pass of ONE wave (rare: only after a poisoned or tiny row sum): queries q0 .. q0+nq-1 of one (frame, head) again,
// 32 at a time, with a running maximum per 64-key tile; fragments come straight from global memory in the layouts of the
// main loop (K rows permuted so that a lane holds 8 consecutive keys per 16-key group), no LDS, no barriers.
// TAG: one instantiation per kernel family -- an out-of-line device function is compiled ONCE per instantiation with the
// register budget of its most generous caller, and every caller then inherits that allocation (round 3: next to a
// 256-register kernel the shared safe pass cost the 128-register kernel half its occupancy).
// (safe_pass_impl: the body.  Its only caller is safe_pass, but writing it straight into the __noinline__ function is not a neutral
//  edit: hipcc then compiles the pass differently (fp16: 690 instead of 623 instructions) and, since a caller's register allocation
//  knows what its callee clobbers, attention4_kernel and attention6_kernel change with it (scripts/isa_diff.py).  Fold it only
//  together with a measurement of both kernels.)
template <typename T>
__device__ __forceinline__ void safe_pass_impl(const T* Qb, const T* Kb, const T* Vb, T* Ob, int q0, int nq, int S, int Sp,
                                               int D) {
    typedef Operand<T> Op;
    typedef typename Op::v8 op8;
    typedef typename Op::v4 op4;
    const int lane = threadIdx.x & 63, lq = lane & 31, hi = lane >> 5;
    const int krow = (lq & 19) | ((lq & 4) << 1) | ((lq & 8) >> 1);
    const int ntiles = (S + 63) / 64;
#pragma unroll 1
    for (int qq = q0; qq < q0 + nq; qq += 32) {
        op8 qf[4];
        const int qrow = min(qq + lq, Sp - 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const op8*>(Qb + (size_t)qrow * 64 + ks * 16 + hi * 8);
        f16v oa[2];
        float m = -3e38f;
        f2 l = {0.f, 0.f};
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) oa[db][r] = 0.f;
#pragma unroll 1
        for (int t = 0; t < ntiles; ++t) {
            f16v s2[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s2[b][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const op8 kf = *reinterpret_cast<const op8*>(Kb + (size_t)(t * 64 + b * 32 + krow) * 64 + ks * 16 + hi * 8);
                    s2[b] = Op::mfma(kf, qf[ks], s2[b]);
                }
            }
            float tm = -3e38f;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t * 64 + b * 32 + 16 * (r >> 3) + 8 * hi + (r & 7);
                    if (key >= S) s2[b][r] = -1e30f;
                    tm = fmaxf(tm, s2[b][r]);
                }
            tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
            const float mn = fmaxf(m, tm);
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            m = mn;
            l *= f2{alpha, alpha};
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) oa[db][r] *= alpha;
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) {
                op8 pfr;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float pv = __builtin_amdgcn_exp2f(s2[bj >> 1][8 * (bj & 1) + e] - m);
                    l[e & 1] += pv;
                    pfr[e] = (T)pv;
                }
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    const op8 vf = *reinterpret_cast<const op8*>(Vb + (size_t)(db * 32 + lq) * Sp + t * 64 + bj * 16 + hi * 8);
                    oa[db] = Op::mfma(vf, pfr, oa[db]);
                }
            }
        }
        const float lh = l[0] + l[1];
        const float inv = 1.f / (lh + __shfl_xor(lh, 32, 64));
        const int qi = qq + lq;
        if (qi < S) {
            T* orow = Ob + (size_t)qi * D;
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const int d = db * 32 + 8 * rq + 4 * hi;
                    op4 v = {(T)(oa[db][4 * rq + 0] * inv), (T)(oa[db][4 * rq + 1] * inv), (T)(oa[db][4 * rq + 2] * inv),
                             (T)(oa[db][4 * rq + 3] * inv)};
                    *reinterpret_cast<op4*>(orow + d) = v;
                }
        }
    }
}
template <typename T, int TAG>
__device__ __noinline__ void safe_pass(const T* Qb, const T* Kb, const T* Vb, T* Ob, int q0, int nq, int S, int Sp, int D) {
    safe_pass_impl(Qb, Kb, Vb, Ob, q0, nq, S, Sp, D);
}

// O^T += A B with the accumulator PINNED to the AGPR half of the register file.  The O accumulators (64 registers) are only
// ever touched by these MFMAs (and by the rare rescale / the epilogue), so with them in AGPRs everything the VALU works on
// -- scores, P, the fragment registers -- fits the 256 architectural VGPRs; left to the register allocator (builtin MFMA,
// -amdgpu-mfma-vgpr-form) the accumulators wandered between the two halves through v_accvgpr copies inside the key loop.
// The compiler's hazard recognizer does not see through an asm statement: the only instructions that read these registers
// outside the MFMAs themselves are behind agpr_settle() below.
template <typename T>
__device__ __forceinline__ void mfma_acc_agpr(f16v& c, typename Operand<T>::v8 a, typename Operand<T>::v8 b) {
    if constexpr (Operand<T>::F16) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
// an MFMA result is read by a non-MFMA instruction: 16-pass MFMA -> up to 18 wait states (and more for a dependent chain in flight)
__device__ __forceinline__ void agpr_settle() { asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory"); }

}  // namespace attn
