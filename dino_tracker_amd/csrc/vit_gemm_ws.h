// vit_gemm_ws.h -- the weight-stationary GEMM of the ViT encoder for K = 384 (QKV, attention projection and fc1 of ViT-S).
#pragma once
#include <utility>
#include "vit_gemm_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// weight-stationary GEMM for K = 384 (QKV, attention projection and fc1 of ViT-S): C[M][N] = A[M][384] . Wt[N][384]^T
//
// A workgroup of two waves owns 128 output features for a chunk of token tiles; a wave keeps its 64 weight rows in
// registers for the whole chunk (A operand of MFMA 32x32x16 bf16: 24 k-steps x 2 row tiles = 192 VGPRs) and the tokens
// stream through a triple-buffered LDS tile of 32 tokens (24 KB) filled by LDS-DMA two steps ahead, read once per wave
// as the B operand: one ds_read_b128 feeds two MFMAs and there is no K loop with barriers -- one barrier per 32 tokens.
// The weight rows are permuted over the MFMA rows so that in D a lane (token j, half h) holds 16 CONSECUTIVE output
// features (n0 + 32 t + 16 h + r): the epilogue of the previous tile (bias, GELU / Q scale / LayerScale, conversion,
// 16-byte stores) is issued between the MFMAs of the current one.  Two workgroups share a CU (one wave per SIMD).
// Measured alternatives (all slower on MI355X): staging the outputs through LDS for whole-line stores, one output
// feature per lane (2-byte stores), 4 tokens x 256 B per DMA request, register-staged tiles instead of LDS-DMA.
// ---------------------------------------------------------------------------------------------------------------
constexpr int WS_KS = 24, WS_K = 16 * WS_KS, WS_ROWS = 32, WS_COLS = 256;
constexpr int WS_TILE_BYTES = WS_ROWS * WS_K * 2;
constexpr int WS_LQ = WS_KS / 4;  // LDS-DMA requests per wave per tile
constexpr int WS_PITCH = 144;                    // staging row pitch: 128 B of payload + 16 (conflict-free 16-B accesses)
constexpr int WS_UNIT_BYTES = WS_ROWS * WS_PITCH;  // staging unit: 32 rows x 128 B (64 bf16 or 32 fp32 outputs)

// V2M (round 4, default 3): bit 0 = weights in AGPRs (loaded there by asm; the builtin MFMA takes them from there as they are)
// and zero accumulators through the MFMA's C operand; bit 1 = token tiles by LDS-DMA through a buffer descriptor (scalar tile
// offset + constant per-lane offset: 3 issue slots per request instead of ~13).  V2M = 0 is the round 1-3 form, kept for the
// A / B measurement (DTK_VIT_GEMM_WS_V1).  Same-box A / B: proj 4.97 -> 3.62 ms, qkv 12.34 -> 12.10, fc1 14.68 -> 14.55 ms per step.
template <typename T, int EPI, int V2M = 3>
__global__ __launch_bounds__(256) void gemm_ws_kernel(const T* __restrict__ A, const T* __restrict__ Wt,
                                                      long long M, int N, GemmEpi<T> e, int tiles_per_chunk) {
    typedef typename Vec<T>::t8 T8;
    typedef typename Vec<T>::t4 T4;
    (void)sizeof(T8); (void)sizeof(T4);
    constexpr bool V2 = (V2M & 1) != 0;       // AGPR weights + zero C operand
    constexpr bool V2D = (V2M & 2) != 0;      // descriptor LDS-DMA
    operand_mode<T>();
    __shared__ __attribute__((aligned(1024))) unsigned char toks[3][WS_TILE_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char stage[4][2][WS_UNIT_BYTES];  // per wave: two staging units
    __shared__ __attribute__((aligned(16))) float s_bias[4][64], s_gamma[4][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * WS_COLS + w * 64;
    const long long total_tiles = (M + WS_ROWS - 1) / WS_ROWS;
    const long long tile0 = (long long)blockIdx.y * tiles_per_chunk;
    if (tile0 >= total_tiles) return;
    const int NT = (int)((total_tiles - tile0) < tiles_per_chunk ? (total_tiles - tile0) : tiles_per_chunk);
    // weights: MFMA row i of row tile t carries output feature n0 + 32 t + nl(i), nl chosen so that D row
    // (r & 3) + 8 (r >> 2) + 4 h  <->  feature 16 h + r
    const int nl = (j & 3) + 4 * (j >> 3) + 16 * ((j >> 2) & 1);
    T8 wf[2][WS_KS];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int row = min(n0 + t * 32 + nl, N - 1);
        const T* wp = Wt + (size_t)row * WS_K + h * 8;
#pragma unroll
        for (int ks = 0; ks < WS_KS; ++ks) {
            if (V2) asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(wf[t][ks]) : "v"(wp + ks * 16) : "memory");
            else wf[t][ks] = *reinterpret_cast<const T8*>(wp + ks * 16);
        }
    }
    if (V2) {
        // the loads above are invisible to the compiler's own vmcnt bookkeeping: wait, then re-define every loaded register behind
        // the wait (an empty volatile asm with a "+a" operand emits nothing, but volatile asms keep their order and no use of
        // wf can be scheduled above its re-definition -- ADVICE r4: before, only scheduling luck kept uses behind the wait)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int ks = 0; ks < WS_KS; ++ks) asm volatile("" : "+a"(wf[t][ks]));
    }
    {
        const int n = min(n0 + lane, N - 1);
        s_bias[w][lane] = e.bias ? e.bias[n] : 0.f;
        s_gamma[w][lane] = (EPI == EPI_DELTA) ? e.gamma[n] : 1.f;
    }
    // QKV: a 64-feature group is one head of q, k or v
    const int which = (EPI == EPI_QKV) ? min(n0, N - 1) / e.D : 0;  // (the last column group of N = 1152 / 384 has idle waves)
    const int head = (EPI == EPI_QKV) ? (min(n0, N - 1) - which * e.D) >> 6 : 0;
    const float qsc = (EPI == EPI_QKV && which == 0) ? e.qscale : 1.f;
    // this lane's token of the tile whose epilogue runs next, as (frame, position) for the QKV layouts
    long long m_ep = tile0 * WS_ROWS + j;
    int f_ep = 0, s_ep = 0;
    if (EPI == EPI_QKV) { f_ep = (int)(m_ep / e.S); s_ep = (int)(m_ep - (long long)f_ep * e.S); }
    // token tiles: a DMA request fetches 4 tokens x 256 contiguous bytes (8 cache lines; one token row per lane would be
    // 32).  Region (g, c) of 1 KB holds tokens 4g .. 4g+3, pieces 16c .. 16c+15 (piece = 8 k values); piece pp of token
    // tt sits at slot ((pp + g) & 15) * 4 + tt, which keeps the fragment reads of 16 consecutive lanes conflict-free
    const unsigned lds_base = (unsigned)(size_t)&toks[0][0];
    const int l_tt = lane & 3, l_pp = lane >> 2;
    // V2: descriptor over the chunk's first token row (32-bit offsets inside a chunk: tiles_per_chunk x 24 KB)
    const dtk_u4 srd = dtk_make_srd(A + tile0 * WS_ROWS * WS_K);
    // (rows of the LAST token tile past M - 1 read row M - 1, as the 64-bit form did: a second pair of offsets for that tile)
    unsigned a_voff[2], a_voff_last[2];
    const int last_rows = (int)(M - (total_tiles - 1) * WS_ROWS);   // valid rows of the last tile (1 .. 32)
#pragma unroll
    for (int gg = 0; gg < 2; ++gg) {
        const int g = 2 * w + gg;
        a_voff[gg] = (unsigned)(((4 * g + l_tt) * WS_K + ((l_pp - g) & 15) * 8) * 2);
        a_voff_last[gg] = (unsigned)((min(4 * g + l_tt, last_rows - 1) * WS_K + ((l_pp - g) & 15) * 8) * 2);
    }
    const unsigned a_dst = __builtin_amdgcn_readfirstlane(lds_base + (2 * w) * 3 * 1024);
    auto issue = [&](int n, int buf) {
        if (V2D) {
            const unsigned toff = __builtin_amdgcn_readfirstlane((unsigned)n * (unsigned)WS_TILE_BYTES);
            const unsigned dst = __builtin_amdgcn_readfirstlane(a_dst + (unsigned)buf * (unsigned)WS_TILE_BYTES);
            const bool last = tile0 + n == total_tiles - 1;
            const unsigned v0 = last ? a_voff_last[0] : a_voff[0], v1 = last ? a_voff_last[1] : a_voff[1];
            dtk_buffer_lds16<0>(srd, toff, v0, dst);
            dtk_buffer_lds16<1024>(srd, toff + 256u, v0, dst);
            dtk_buffer_lds16<2048>(srd, toff + 512u, v0, dst);
            dtk_buffer_lds16<3072>(srd, toff, v1, dst);
            dtk_buffer_lds16<4096>(srd, toff + 256u, v1, dst);
            dtk_buffer_lds16<5120>(srd, toff + 512u, v1, dst);
            return;
        }
#pragma unroll
        for (int gg = 0; gg < 2; ++gg) {
            const int g = 2 * w + gg;
            const long long m = min((tile0 + n) * WS_ROWS + 4 * g + l_tt, M - 1);
            const T* gp = A + m * WS_K + ((l_pp - g) & 15) * 8;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                dtk_glds16(gp + c * 128, __builtin_amdgcn_readfirstlane(lds_base + buf * WS_TILE_BYTES + (g * 3 + c) * 1024));
        }
    };
    // B-operand fragment of k-step ks for lane (token j, half h): piece 2 ks + h -> region column c = ks >> 3
    unsigned frag_off[8];
#pragma unroll
    for (int k8 = 0; k8 < 8; ++k8)
        frag_off[k8] = (unsigned)((j >> 2) * 3 * 1024 + ((((2 * k8 + h + (j >> 2)) & 15) * 4 + (j & 3)) * 16));
    // epilogue of 8 values (row tile t, half hv of this lane's 16 features): features nb .. nb + 7
    float amax = 0.f;
    auto epi8 = [&](const f16v (&acc)[2], int t, int hv) {
        const int fl = 32 * t + 16 * h + 8 * hv;  // feature offset inside the wave's 64
        const int nb = n0 + fl;
        const float4 b0 = *reinterpret_cast<const float4*>(&s_bias[w][fl]), b1 = *reinterpret_cast<const float4*>(&s_bias[w][fl + 4]);
        float v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = acc[t][8 * hv + r];
        v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w;
        v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
        const bool ok = m_ep < M && nb < N && !DTK_DBG(e.no_store, 3);
        if (IsF16<T>::value && (EPI == EPI_QKV || EPI == EPI_GELU)) {   // the fp16 range, every value of every frame (GemmEpi::ovf)
#pragma unroll
            for (int r = 0; r < 8; r += 2) {
                if (EPI == EPI_GELU) amax = fmaxf(fmaxf(amax, v[r]), v[r + 1]);   // the stored GELU(v): the positive part of v
                else amax = amax2(amax, v[r] * qsc, v[r + 1] * qsc);
            }
        }
        if (EPI == EPI_GELU) {
            T8 o;
#pragma unroll
            for (int r = 0; r < 8; r += 2) {
                const f2 g = gelu2(f2{v[r], v[r + 1]});
                o[r] = (T)g[0];
                o[r + 1] = (T)g[1];
            }
            // (staging the GELU output for whole-line stores measured slower than these scattered 16-byte stores)
            if (ok) *reinterpret_cast<T8*>(e.out + m_ep * N + nb) = o;
        } else if (EPI == EPI_DELTA) {
            const float4 g0 = *reinterpret_cast<const float4*>(&s_gamma[w][fl]), g1 = *reinterpret_cast<const float4*>(&s_gamma[w][fl + 4]);
            T8 o = {(T)(v[0] * g0.x), (T)(v[1] * g0.y), (T)(v[2] * g0.z), (T)(v[3] * g0.w),
                     (T)(v[4] * g1.x), (T)(v[5] * g1.y), (T)(v[6] * g1.z), (T)(v[7] * g1.w)};
            *reinterpret_cast<T8*>(&stage[w][0][0] + j * WS_PITCH + fl * 2) = o;
        } else {
            const int dh = fl;  // 0..63 inside the head
            if (which == 2) {
                // V^T[f][head][dh][s]: consecutive lanes are consecutive tokens
                // (round 6, measured and dropped: staging the wave's 64 x 32 tile transposed in LDS and flushing 8-byte pieces of four
                //  tokens -- 8 store instructions instead of 32 -- made qkv 12.3 -> 15.7 ms per step: the 32 two-byte LDS writes sit in
                //  the lone wave's issue stream like the stores they replace; docs/NEGATIVE_RESULTS.md)
                if (ok) {
                    T* vp = e.vt + (((size_t)f_ep * e.heads + head) * 64 + dh) * e.Sp + s_ep;
#pragma unroll
                    for (int r = 0; r < 8; ++r) vp[(size_t)r * e.Sp] = (T)v[r];
                }
            } else {
                T8 o;
#pragma unroll
                for (int r = 0; r < 8; ++r) o[r] = (T)(v[r] * qsc);
                *reinterpret_cast<T8*>(&stage[w][0][0] + j * WS_PITCH + fl * 2) = o;
            }
        }
    };
    // staged rows -> global memory with 8 lanes per 128-byte output row (whole lines).  (mt_fl, f0_fl, s0_fl): first
    // token of the staged tile and its (frame, position)
    long long mt_fl = tile0 * WS_ROWS;
    int f0_fl = 0, s0_fl = 0;
    if (EPI == EPI_QKV) { f0_fl = (int)(mt_fl / e.S); s0_fl = (int)(mt_fl - (long long)f0_fl * e.S); }
    auto flush = [&]() {
        if (EPI != EPI_GELU && n0 < N && !DTK_DBG(e.no_store, 3) && !(EPI == EPI_QKV && which == 2)) {
#pragma unroll
            for (int u = 0; u < 1; ++u) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int row = 8 * p + (lane >> 3), piece = lane & 7;
                    const uint4 val = *reinterpret_cast<const uint4*>(&stage[w][u][0] + row * WS_PITCH + piece * 16);
                    if (mt_fl + row < M) {
                        if (EPI == EPI_DELTA) {
                            *reinterpret_cast<uint4*>(e.delta + (mt_fl + row) * N + n0 + piece * 8) = val;
                        } else {
                            int f = f0_fl, sp = s0_fl + row;  // a tile crosses at most one frame end
                            if (sp >= e.S) { sp -= e.S; ++f; }
                            T* dst = which == 0 ? e.q : e.k;
                            *reinterpret_cast<uint4*>(dst + (((size_t)f * e.heads + head) * e.Sp + sp) * 64 + piece * 8) = val;
                        }
                    }
                }
            }
        }
        mt_fl += WS_ROWS;
        if (EPI == EPI_QKV) {
            s0_fl += WS_ROWS;
            if (s0_fl >= e.S) { s0_fl -= e.S; ++f0_fl; }
        }
    };
    auto advance = [&]() {  // the epilogue moves on to the next tile
        m_ep += WS_ROWS;
        if (EPI == EPI_QKV) {
            s_ep += WS_ROWS;
            if (s_ep >= e.S) { s_ep -= e.S; ++f_ep; }
        }
    };
    // one step: MFMAs of the tile in `buf` into accN, with the four epilogue pieces of the previous tile (accP) in between
    auto step = [&](int buf, f16v (&accN)[2], const f16v (&accP)[2], bool have_prev, bool have_flush) {
        if (!V2) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) accN[t][r] = 0.f;
        }
        const unsigned char* base = &toks[0][0] + buf * WS_TILE_BYTES;
        const f16v zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // inline constant C
        T8 b[3];
        b[0] = *reinterpret_cast<const T8*>(base + frag_off[0]);
        b[1] = *reinterpret_cast<const T8*>(base + frag_off[1]);
#pragma unroll
        for (int ks = 0; ks < WS_KS; ++ks) {
            if (ks + 2 < WS_KS)
                b[(ks + 2) % 3] = *reinterpret_cast<const T8*>(base + frag_off[(ks + 2) & 7] + ((ks + 2) >> 3) * 1024);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                // (V2: the builtin, NOT an asm MFMA: its A operand accepts the AGPR the weight was loaded into as it is, and the
                // compiler keeps managing the instruction's hazards -- an asm MFMA followed by compiler-scheduled code that
                // re-used its B registers for an LDS load at once gave wrong tokens, non-deterministically)
                if (V2) accN[t] = mfma32(wf[t][ks], b[ks % 3], ks == 0 ? zero16 : accN[t]);
                else accN[t] = mfma32(wf[t][ks], b[ks % 3], accN[t]);
            }
            // the tile staged during the previous step leaves first: its stores have the whole step to retire
            if (have_flush && ks == 0) flush();
            if (have_prev && ks % 6 == 2) epi8(accP, (ks / 6) >> 1, (ks / 6) & 1);
        }
        if (have_prev) advance();
    };
    f16v accA[2], accB[2];
    // three LDS buffers, tiles requested two steps ahead.  The wait at the end of a step must prove that the tile of the
    // next step has landed: loads retire in order among themselves and the stores of the epilogue only add to the
    // count, so vmcnt(LQ) -- the requests of the tile after next -- is sufficient, if conservative.
    issue(0, 0);
    issue(min(1, NT - 1), 1);
    dtk_vm_wait<WS_LQ>();
    __syncthreads();
    int n = 0, b0 = 0;
    for (; n + 1 < NT; n += 2) {
        const int b1 = b0 == 2 ? 0 : b0 + 1, b2 = b1 == 2 ? 0 : b1 + 1;
        issue(min(n + 2, NT - 1), b2);
        step(b0, accA, accB, n > 0, n > 1);
        dtk_vm_wait<WS_LQ>();
        __syncthreads();
        issue(min(n + 3, NT - 1), b0);
        step(b1, accB, accA, true, n > 0);
        dtk_vm_wait<WS_LQ>();
        __syncthreads();
        b0 = b2;
    }
    if (n < NT) {  // NT odd: one more tile
        step(b0, accA, accB, n > 0, n > 1);
        if (n > 0) flush();
#pragma unroll
        for (int u = 0; u < 4; ++u) epi8(accA, u >> 1, u & 1);
    } else {
        if (n > 1) flush();
#pragma unroll
        for (int u = 0; u < 4; ++u) epi8(accB, u >> 1, u & 1);
    }
    flush();
    amax_report<T, EPI>(amax, e.ovf);
    dtk_vm_wait<0>();
}

// grid (column workgroups, token chunks) and token tiles per chunk: one resident round, one workgroup per CU
inline std::pair<dim3, int> gemm_ws_grid(int N, long long rows) {
    const int colwg = dtk_cdiv(N, WS_COLS);
    const int chunks = 256 / colwg > 0 ? 256 / colwg : 1;
    const long long tiles = dtk_cdiv(rows, WS_ROWS);
    const int tpc = (int)dtk_cdiv(tiles, chunks);
    return std::make_pair(dim3(colwg, (unsigned)dtk_cdiv(tiles, tpc)), tpc);
}

}  // namespace
