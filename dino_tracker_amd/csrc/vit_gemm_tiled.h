// vit_gemm_tiled.h -- the 128 x 128 register-staged GEMM of the ViT encoder: every shape, every epilogue (the cross-check of the
// faster forms, DTK_VIT_TILED_GEMMS, and the fp32 qkv facet).
#pragma once
#include "vit_gemm_common.h"

namespace {

// (Round 2 measured two LDS-DMA forms of this main loop on fc2, K = 1536: 64-wide stages, two in flight, two barriers per
// stage: 17.9 ms; 32-wide stages in a ring of four, three in flight, one barrier per stage: 20.0 ms; this register-staged
// form: 17.1-17.5 ms.  Kept.  The SQ counters (profiles/r02_pmc_sq.md) show why it is slow -- 64 % of the wave cycles
// parked, MFMA pipe 27 % busy: one k-step of prefetch does not cover the HBM latency -- but TWO k-steps of register
// prefetch need 150 VGPRs = 3 waves per SIMD instead of 4 and measured 18.7 ms; forced to 128 VGPRs the loop spills.)
template <typename T, int EPI>
__global__ __launch_bounds__(256) void gemm_tiled_kernel(const T* __restrict__ A, const T* __restrict__ Wt,
                                                         long long M, int N, int K, GemmEpi<T> e) {
    typedef typename Vec<T>::t8 T8;
    typedef typename Vec<T>::t4 T4;
    (void)sizeof(T8); (void)sizeof(T4);
    operand_mode<T>();
    __shared__ uint4 As[2][GM * 4];
    __shared__ uint4 Bs[2][GN * 4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // block -> tile: workgroup b runs on XCD b % 8 (round-robin dispatch); the column tiles of one row block are given
    // to the same XCD back to back, so that A is fetched from HBM once and the other N/128 - 1 reads hit that XCD's L2
    // (with column-major block order fc2 re-read its 0.75 GB operand three times: 5.2 TB/s, HBM-bound)
    const int ncol = (N + GN - 1) / GN;
    const long long nrow = (M + GM - 1) / GM;
    const long long kb = blockIdx.x >> 3;
    const long long row_blk = (kb / ncol) * 8 + (blockIdx.x & 7);
    if (row_blk >= nrow) return;
    const long long m0 = row_blk * GM;
    const int n0 = (int)(kb % ncol) * GN;
    const int wr = w >> 1, wc = w & 1;  // wave tile 64 x 64
    const int fj = lane & 15, fg = lane >> 4;
    const int lrow = tid >> 2, lpiece = tid & 3;  // loader rows lrow, lrow + 64
    // clamp loader rows so that ragged M / N never read out of bounds (results of clamped rows are not stored)
    const long long ar0 = min(m0 + lrow, M - 1), ar1 = min(m0 + lrow + 64, M - 1);
    const int br0 = min(n0 + lrow, N - 1), br1 = min(n0 + lrow + 64, N - 1);
    const T* a0 = A + ar0 * K + lpiece * 8;
    const T* a1 = A + ar1 * K + lpiece * 8;
    const T* b0 = Wt + (size_t)br0 * K + lpiece * 8;
    const T* b1 = Wt + (size_t)br1 * K + lpiece * 8;
    f4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f4{0.f, 0.f, 0.f, 0.f};
    uint4 ra0 = *reinterpret_cast<const uint4*>(a0), ra1 = *reinterpret_cast<const uint4*>(a1);
    uint4 rb0 = *reinterpret_cast<const uint4*>(b0), rb1 = *reinterpret_cast<const uint4*>(b1);
    As[0][gswz(lrow, lpiece)] = ra0;
    As[0][gswz(lrow + 64, lpiece)] = ra1;
    Bs[0][gswz(lrow, lpiece)] = rb0;
    Bs[0][gswz(lrow + 64, lpiece)] = rb1;
    __syncthreads();
    const int nk = K / GK;
    int cur = 0;
    for (int ks = 0; ks < nk; ++ks) {
        if (ks + 1 < nk) {
            ra0 = *reinterpret_cast<const uint4*>(a0 + (ks + 1) * GK);
            ra1 = *reinterpret_cast<const uint4*>(a1 + (ks + 1) * GK);
            rb0 = *reinterpret_cast<const uint4*>(b0 + (ks + 1) * GK);
            rb1 = *reinterpret_cast<const uint4*>(b1 + (ks + 1) * GK);
        }
        T8 af[4], bfr[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const uint4 v = As[cur][gswz(wr * 64 + mi * 16 + fj, fg)];
            af[mi] = *reinterpret_cast<const T8*>(&v);
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const uint4 v = Bs[cur][gswz(wc * 64 + ni * 16 + fj, fg)];
            bfr[ni] = *reinterpret_cast<const T8*>(&v);
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                acc[mi][ni] = mfma16(af[mi], bfr[ni], acc[mi][ni]);
        if (ks + 1 < nk) {
            As[cur ^ 1][gswz(lrow, lpiece)] = ra0;
            As[cur ^ 1][gswz(lrow + 64, lpiece)] = ra1;
            Bs[cur ^ 1][gswz(lrow, lpiece)] = rb0;
            Bs[cur ^ 1][gswz(lrow + 64, lpiece)] = rb1;
        }
        __syncthreads();
        cur ^= 1;
    }
    // D fragment: lane (fg, fj) holds rows 4*fg + r (r = 0..3), column fj of each 16x16 tile
    float amax = 0.f;
    if constexpr (EPI == EPI_SWIGLU) {   // (N = 8192: whole tiles) gate fragments ni = 0, 1 with their value fragments ni + 2
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int n = n0 + wc * 64 + ni * 16 + fj;
            const float bg = e.bias ? e.bias[n] : 0.f, bv = e.bias ? e.bias[n + 32] : 0.f;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                gemm_store_tile_swiglu<T>(acc[mi][ni], acc[mi][ni + 2], m0 + wr * 64 + mi * 16 + fg * 4, n, bg, bv, M, N, e, amax);
        }
        amax_report<T, EPI>(amax, e.ovf);
        return;
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int n = n0 + wc * 64 + ni * 16 + fj;
        if (n >= N) continue;
        const float bias = e.bias ? e.bias[n] : 0.f;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const long long mb = m0 + wr * 64 + mi * 16 + fg * 4;
            gemm_store_tile<T, EPI>(acc[mi][ni], mb, n, bias, M, N, e, amax);
        }
    }
    amax_report<T, EPI>(amax, e.ovf);
}

// 1-D grid of gemm_tiled_kernel: 8 row blocks (one per XCD) x all column tiles per group
inline unsigned gemm_grid(int N, long long rows) {
    const long long ncol = dtk_cdiv(N, GN), nrow = dtk_cdiv(rows, GM);
    return (unsigned)(dtk_cdiv(nrow, 8) * 8 * ncol);
}

}  // namespace
