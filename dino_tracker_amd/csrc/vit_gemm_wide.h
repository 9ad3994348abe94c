// vit_gemm_wide.h -- the LDS-DMA pipelined GEMMs of the ViT encoder: 256 x 384 tiles for fc2 of ViT-S (gemm_wide_delta_kernel) and
// 256 x 256 tiles for every GEMM of the wider models (gemm_wide_kernel).
#pragma once
#include <type_traits>
#include "vit_gemm_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// wide-tile GEMM for N = 384 and long K (fc2 of ViT-S: K = 1536):  C[M][384] = A[M][K] . Wt[384][K]^T, EPI_DELTA epilogue
//
// The 128x128 kernel above is bound by memory LATENCY, not bandwidth: a CU streams 16 KB per k-step and would need
// ~200 KB in flight to cover ~1.5 us, its 16 waves stage 64 KB (SQ counters: waves parked 64 %, MFMA pipe 27 % busy).
// Here one workgroup of 8 waves owns 256 rows x ALL 384 columns: A is read exactly once (no column tiles), a k-step
// moves 40 KB for 6.3 MFLOP (2.4x fewer bytes per flop), and the tiles arrive by LDS-DMA (global_load_lds_dwordx4, no
// staging registers) into a ring of three 40 KB stages, two of them in flight -- 80 KB per CU against the ~93 KB that
// Little's law asks for at this intensity.  LDS image = the 128x128 kernel's (row-major, four 16-byte pieces per row,
// piece XOR-swizzled by gswz), produced by giving every DMA lane the matching SOURCE address.  One barrier per k-step.
// Wave grid 2 x 4, wave tile 128 x 96 = 8 x 6 MFMA 16x16x32 tiles: 192 accumulator registers, two waves per SIMD.
// (For the attention projection, K = 384 = 12 k-steps, the pipeline's fill time dominates: 6.9 ms against 5.4 ms on the
// weight-stationary kernel.  fc2 only.)
// ---------------------------------------------------------------------------------------------------------------
constexpr int WD_M = 256, WD_N = 384, WD_STAGES = 3;
constexpr int WD_A_BYTES = WD_M * 64, WD_B_BYTES = WD_N * 64, WD_STAGE_BYTES = WD_A_BYTES + WD_B_BYTES;
constexpr int WD_REQ = (WD_M + WD_N) / 16 / 8;  // DMA requests per wave and stage (16 rows of 64 B each): 5
constexpr int WD_OPITCH = WD_N * 2 + 8;   // staged output rows (round 6): 768 B + 8
static_assert(128 * WD_OPITCH <= WD_STAGES * WD_STAGE_BYTES, "a staged half tile must fit the stages");

template <typename T, bool STAGED = true, bool FUSE_LN = false>
__global__ __launch_bounds__(512, 2) void gemm_wide_delta_kernel(const T* __restrict__ A, const T* __restrict__ Wt,
                                                                 long long M, int K, GemmEpi<T> e) {
    typedef typename Vec<T>::t8 T8;
    typedef typename Vec<T>::t4 T4;
    (void)sizeof(T8); (void)sizeof(T4);
    operand_mode<T>();
    __shared__ __attribute__((aligned(1024))) unsigned char stages[WD_STAGES * WD_STAGE_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long m0 = (long long)blockIdx.x * WD_M;
    const int wr = w >> 2, wc = w & 3;  // wave tile: rows wr*128.., columns wc*96..
    const int fj = lane & 15, fg = lane >> 4;
    // ---- DMA sources: request q = 5 w + i covers 16 rows (A rows 16q.. for q < 16, Wt rows 16(q-16).. otherwise); lane
    // (row 16q' + lane/4, slot lane%4) fetches the piece that gswz puts in that slot
    dtk_u4 srd[WD_REQ];
    unsigned voff[WD_REQ];
#pragma unroll
    for (int i = 0; i < WD_REQ; ++i) {
        const int q = w * WD_REQ + i;
        const bool isA = q < WD_M / 16;
        const int row = (isA ? q : q - WD_M / 16) * 16 + (lane >> 2);
        const int piece = (lane & 3) ^ ((0x1230 >> (((row >> 2) & 3) * 4)) & 3);   // gswz_f(row) spelled out: the call changes the code
        const int trow = isA ? (int)(min(m0 + row, M - 1) - m0) : row;  // Wt has exactly WD_N rows; rows past M repeat the last one
        srd[i] = dtk_make_srd(isA ? A + m0 * K : Wt);
        voff[i] = (unsigned)(trow * K + piece * 8) * 2u;
    }
    const unsigned lds0 = (unsigned)(size_t)&stages[0] + (unsigned)w * (WD_REQ * 1024);
    const int nk = K / GK;
    auto issue = [&](int ks, int buf) {
        const int kk = min(ks, nk - 1);  // past the end: a harmless repeat keeps the request count per stage uniform
        wd_issue<WD_REQ>(srd, voff, (unsigned)kk * (GK * 2), __builtin_amdgcn_readfirstlane(lds0 + buf * WD_STAGE_BYTES));
    };
    f4 acc[8][6];
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 6; ++ni) acc[mi][ni] = f4{0.f, 0.f, 0.f, 0.f};
    // fragment addresses: row (tile row 16 mi + fj) -> uint4 index row * 4 + (fg ^ f(row)); f depends on fj only
    const int fsw = gswz_f(fj);
    const unsigned a_off = ((wr * 128 + fj) * 4 + (fg ^ fsw)) * 16;
    const unsigned b_off = WD_A_BYTES + ((wc * 96 + fj) * 4 + (fg ^ fsw)) * 16;
    issue(0, 0);
    issue(1, 1);
    dtk_vm_wait<WD_REQ>();  // stage 0 landed (stage 1 may still fly)
    __syncthreads();
    int buf = 0;
    for (int ks = 0; ks < nk; ++ks) {
        const int nxt2 = buf == 0 ? 2 : buf - 1;  // (buf + 2) % 3: the stage consumed in the previous iteration
        issue(ks + 2, nxt2);
        const unsigned char* sb = stages + buf * WD_STAGE_BYTES;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            T8 af[4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                af[mi] = *reinterpret_cast<const T8*>(sb + a_off + (half * 4 + mi) * 1024);
#pragma unroll
            for (int ni = 0; ni < 6; ++ni) {
                const T8 bfr = *reinterpret_cast<const T8*>(sb + b_off + ni * 1024);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    acc[half * 4 + mi][ni] =
                        mfma16(bfr, af[mi], acc[half * 4 + mi][ni]);   // (W tile) x (token tile)^T: D transposed (round 5), see the epilogue
            }
        }
        dtk_vm_wait<WD_REQ>();  // stage ks + 1 landed; the requests of ks + 2 stay in flight
        __syncthreads();
        buf = buf == 2 ? 0 : buf + 1;
    }
    dtk_vm_wait<0>();
    // D tiles are TRANSPOSED (round 5): lane (fg, fj) holds features 4 fg + r (r = 0..3) of token fj of each 16 x 16 tile -- four
    // consecutive features of one token: ONE 8-byte store per tile and lane (48 per lane and 256 x 384 tile) where the
    // token-major form needed four 2-byte stores (192)
    float no_amax = 0.f;   // (EPI_DELTA stores nothing whose range is tracked)
    if (STAGED && FUSE_LN) {
        // Round 6: fc2's epilogue + the NEXT block's LayerNorm.  Two passes; pass p stages the token tiles mi = 4 p .. 4 p + 3 of EVERY
        // wave (rows wr 128 + 64 p .. + 63 of the tile: every wave frees half of its accumulators per pass, which is what leaves
        // registers for the rows of x below) as the same 16-bit delta the unfused path stores.  Then a wave takes 16 of the pass's 128
        // rows, eight at a time: x of the eight rows is requested first, then row by row x += delta, x written back, statistics and
        // the normalised 16-bit row by layernorm_kernel's own expressions and lane -> column map (lane c: columns 4 c .. 4 c + 3, lanes
        // 0-31 also 256 + 4 c ..): bit-identical rows.  The delta tile never reaches memory; one launch and one trip of x + delta per
        // block go away.
        const float4 ga = *reinterpret_cast<const float4*>(e.ln_w + lane * 4), ba = *reinterpret_cast<const float4*>(e.ln_b + lane * 4);
        const float4 gb = *reinterpret_cast<const float4*>(e.ln_w + 256 + (lane & 31) * 4), bb = *reinterpret_cast<const float4*>(e.ln_b + 256 + (lane & 31) * 4);
        bool sat = false;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            __syncthreads();   // p = 0: every wave's requests have landed and the stages are dead; p = 1: pass 0 has been read
#pragma unroll
            for (int ni = 0; ni < 6; ++ni) {
                const int nb = wc * 96 + ni * 16 + fg * 4;
                const float4 b4 = e.bias ? *reinterpret_cast<const float4*>(e.bias + nb) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 g4 = *reinterpret_cast<const float4*>(e.gamma + nb);
#pragma unroll
                for (int mq = 0; mq < 4; ++mq) {
                    const f4& a = acc[4 * p + mq][ni];   // (gemm_value_tile_t<T, EPI_DELTA> spelled out: the call reorders this instantiation's schedule)
                    *reinterpret_cast<T4*>(stages + (wr * 64 + mq * 16 + fj) * WD_OPITCH + nb * 2) =
                        T4{(T)(g4.x * (a[0] + b4.x)), (T)(g4.y * (a[1] + b4.y)), (T)(g4.z * (a[2] + b4.z)), (T)(g4.w * (a[3] + b4.w))};
                }
            }
            __syncthreads();
            // local rows lr0 .. lr0 + NB - 1 of the pass <-> tile rows (lr >> 6) 128 + 64 p + (lr & 63); NB rows of x in flight per wave:
            // 8 while the second half of the accumulators is live (pass 0), 16 in pass 1
            auto ln_rows = [&](auto nb_c, int lr0) {
                constexpr int NB = decltype(nb_c)::value;
                const long long rb = m0 + (lr0 >> 6) * 128 + p * 64 + (lr0 & 63);
                float4 xa[NB], xb[NB];
#pragma unroll
                for (int rr = 0; rr < NB; ++rr) {
                    const float* xp = e.ln_x + min(rb + rr, M - 1) * WD_N + lane * 4;
                    xa[rr] = *reinterpret_cast<const float4*>(xp);
                    xb[rr] = lane < 32 ? *reinterpret_cast<const float4*>(xp + 256) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int rr = 0; rr < NB; ++rr) {
                    const long long row = rb + rr;
                    if (row >= M) continue;   // wave-uniform (the last tile's tail)
                    const unsigned char* sp = stages + (lr0 + rr) * WD_OPITCH + lane * 8;
                    float4 v[2] = {xa[rr], xb[rr]};
                    float s = 0.f;
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        if (it == 0 || lane < 32) {
                            const T4 d = *reinterpret_cast<const T4*>(sp + it * 512);
                            const float d0 = (float)d[0], d1 = (float)d[1], d2 = (float)d[2], d3 = (float)d[3];
                            sat |= update_saturated<T>(d0, d1, d2, d3);
                            v[it].x += d0; v[it].y += d1; v[it].z += d2; v[it].w += d3;
                            *reinterpret_cast<float4*>(e.ln_x + row * WD_N + it * 256 + lane * 4) = v[it];
                            s += (v[it].x + v[it].y) + (v[it].z + v[it].w);
                        }
                    }
                    const float mean = wave_sum(s) / (float)WD_N;
                    float q = 0.f;
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        if (it == 0 || lane < 32) {
                            const float a = v[it].x - mean, b = v[it].y - mean, cc = v[it].z - mean, d = v[it].w - mean;
                            q += (a * a + b * b) + (cc * cc + d * d);
                        }
                    }
                    const float rstd = rsqrtf(wave_sum(q) / (float)WD_N + e.ln_eps);
                    T* o = e.ln_out + row * WD_N;
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        if (it == 0 || lane < 32) {
                            const float4 g = it ? gb : ga, b = it ? bb : ba;
                            T4 r = {(T)((v[it].x - mean) * rstd * g.x + b.x), (T)((v[it].y - mean) * rstd * g.y + b.y),
                                     (T)((v[it].z - mean) * rstd * g.z + b.z), (T)((v[it].w - mean) * rstd * g.w + b.w)};
                            *reinterpret_cast<T4*>(o + it * 256 + lane * 4) = r;
                        }
                    }
                }
            };
            if (p == 0) {
                ln_rows(std::integral_constant<int, 8>{}, w * 16);
                ln_rows(std::integral_constant<int, 8>{}, w * 16 + 8);
            } else {
                ln_rows(std::integral_constant<int, 16>{}, w * 16);
            }
        }
        if (IsF16<T>::value && e.ln_ovf && __any(sat) && lane == 0) atomicOr(e.ln_ovf, 1);
        return;
    }
    if (STAGED) {
        // Round 6: through LDS (see gemm_wide_kernel's epilogue: a CU holds one workgroup of this kernel, nothing overlaps the epilogue,
        // and its 8-byte stores -- 16 tokens x 32 B per instruction -- ran at 1.5 TB/s).  The 256 x 384 tile is 192 KB of 16-bit values:
        // two passes of 128 rows (the waves of row half p stage, everybody writes out: the 128 rows are 96 KB of CONTIGUOUS memory).
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            __syncthreads();   // p = 0: every wave's requests have landed and the stages are dead; p = 1: pass 0 has been read out
            if (wr == p) {
#pragma unroll
                for (int ni = 0; ni < 6; ++ni) {
                    const int nb = wc * 96 + ni * 16 + fg * 4;
                    const float4 b4 = e.bias ? *reinterpret_cast<const float4*>(e.bias + nb) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 g4 = *reinterpret_cast<const float4*>(e.gamma + nb);
#pragma unroll
                    for (int mi = 0; mi < 8; ++mi)
                        *reinterpret_cast<T4*>(stages + (mi * 16 + fj) * WD_OPITCH + nb * 2) = gemm_value_tile_t<T, EPI_DELTA>(acc[mi][ni], b4, g4, no_amax);
                }
            }
            __syncthreads();
            const long long mb = m0 + p * 128;
#pragma unroll 4
            for (int it = 0; it < 128 * (WD_N / 8) / 512; ++it) {   // 6144 16-byte pieces, 12 per thread
                const int idx = it * 512 + tid, row = idx / (WD_N / 8), piece = idx - row * (WD_N / 8);
                const uint4 v = staged16(stages + row * WD_OPITCH + piece * 16);
                if (mb + row < M) *reinterpret_cast<uint4*>(e.delta + (mb + row) * WD_N + piece * 8) = v;
            }
        }
        return;
    }
#pragma unroll
    for (int ni = 0; ni < 6; ++ni) {
        const int nb = wc * 96 + ni * 16 + fg * 4;
        const float4 b4 = e.bias ? *reinterpret_cast<const float4*>(e.bias + nb) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 g4 = *reinterpret_cast<const float4*>(e.gamma + nb);
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) {
            const long long m = m0 + wr * 128 + mi * 16 + fj;
            if (m < M) *reinterpret_cast<T4*>(e.delta + m * WD_N + nb) = gemm_value_tile_t<T, EPI_DELTA>(acc[mi][ni], b4, g4, no_amax);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the same pipeline as a 256 x 256 tile for the GEMMs of wider models (N a multiple of 256: D = 768 / 1024 and their qkv
// / MLP widths), all epilogues.  Stage = 16 KB of A + 16 KB of B, ring of FOUR stages with three in flight (96 KB per
// CU); wave grid 2 x 4, wave tile 128 x 64 = 8 x 4 MFMA tiles (128 accumulator registers).  Block order as in
// gemm_tiled_kernel: the column tiles of a row block run back to back on one XCD.
// ---------------------------------------------------------------------------------------------------------------
constexpr int W2_M = 256, W2_N = 256, W2_STAGES = 4, W2_STAGE_BYTES = (W2_M + W2_N) * 64;
constexpr int W2_REQ = (W2_M + W2_N) / 16 / 8;  // 4 DMA requests per wave and stage
constexpr int W2_OPITCH = W2_N * 2 + 8;          // staged output rows: 512 B + 8 (the 8-byte writes of 16 tokens fall on 16 different bank pairs)
constexpr int W2_LDS_BYTES = W2_STAGES * W2_STAGE_BYTES > W2_M * W2_OPITCH ? W2_STAGES * W2_STAGE_BYTES : W2_M * W2_OPITCH;

inline unsigned gemm_wide_grid(int N, long long rows) {
    const long long ncol = N / W2_N, nrow = dtk_cdiv(rows, W2_M);
    return (unsigned)(dtk_cdiv(nrow, 8) * 8 * ncol);
}

template <typename T, int EPI, bool PIPE = true>
__global__ __launch_bounds__(512, 2) void gemm_wide_kernel(const T* __restrict__ A, const T* __restrict__ Wt,
                                                           long long M, int N, int K, GemmEpi<T> e) {
    typedef typename Vec<T>::t8 T8;
    typedef typename Vec<T>::t4 T4;
    (void)sizeof(T8); (void)sizeof(T4);
    operand_mode<T>();
    __shared__ __attribute__((aligned(1024))) unsigned char stages[W2_LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ncol = N / W2_N;
    const long long nrow = (M + W2_M - 1) / W2_M;
    const long long kb = blockIdx.x >> 3;
    const long long row_blk = (kb / ncol) * 8 + (blockIdx.x & 7);
    if (row_blk >= nrow) return;
    const long long m0 = row_blk * W2_M;
    const int n0 = (int)(kb % ncol) * W2_N;
    const int wr = w >> 2, wc = w & 3;  // wave tile: rows wr*128.., columns wc*64..
    const int fj = lane & 15, fg = lane >> 4;
    dtk_u4 srd[W2_REQ];
    unsigned voff[W2_REQ];
#pragma unroll
    for (int i = 0; i < W2_REQ; ++i) {
        const int q = w * W2_REQ + i;  // 0..15: A rows 16q.., 16..31: Wt rows n0 + 16(q-16)..
        const bool isA = q < W2_M / 16;
        const int row = (isA ? q : q - W2_M / 16) * 16 + (lane >> 2);
        const int piece = (lane & 3) ^ ((0x1230 >> (((row >> 2) & 3) * 4)) & 3);   // gswz_f(row) spelled out: the call changes the code
        const int trow = isA ? (int)(min(m0 + row, M - 1) - m0) : row;
        srd[i] = dtk_make_srd(isA ? A + m0 * K : Wt + (long long)n0 * K);
        voff[i] = (unsigned)(trow * K + piece * 8) * 2u;
    }
    const unsigned lds0 = (unsigned)(size_t)&stages[0] + (unsigned)w * (W2_REQ * 1024);
    const int nk = DTK_DBG(e.no_store, 8) ? 0 : K / GK;
    auto issue = [&](int ks, int buf) {
        const int kk = DTK_DBG(e.no_store, 16 | 8) ? 0 : min(ks, nk - 1);
        wd_issue<W2_REQ>(srd, voff, (unsigned)kk * (GK * 2), __builtin_amdgcn_readfirstlane(lds0 + buf * W2_STAGE_BYTES));
    };
    f4 acc[8][4];
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f4{0.f, 0.f, 0.f, 0.f};
    const int fsw = gswz_f(fj);
    const unsigned a_off = ((wr * 128 + fj) * 4 + (fg ^ fsw)) * 16;
    const unsigned b_off = W2_M * 64 + ((wc * 64 + fj) * 4 + (fg ^ fsw)) * 16;
    issue(0, 0);
    issue(1, 1);
    issue(2, 2);
    dtk_vm_wait<2 * W2_REQ>();  // stage 0 landed
    __syncthreads();
    int buf = 0;
    if (PIPE) {
        // Round 6: the fragment reads run ONE HALF-STEP AHEAD of the MFMAs that consume them.  In the form below every wave reads
        // its eight fragments right behind the barrier -- all eight waves of the CU at once, 64 ds_read_b128 = 256 LDS cycles plus
        // the latency, with the matrix pipes idle (SQ counters, fc2 of ViT-S on the same loop: waves parked 45 %, pipes 38 % busy).
        // Here a k-step is two halves of 16 MFMAs (token tiles 0-3 | 4-7 against the four W tiles); the A fragments of the second
        // half are requested in front of the first half's MFMAs, and A (first half) + W fragments of the NEXT stage behind the
        // barrier, in front of the second half's MFMAs: two fragment sets (fa / fb, alternating with the k-step: the loop is
        // unrolled by two so that the set is a compile-time index), 64 fragment registers + 128 accumulators.
        T8 fa[2][4], fb[2][4], ga[4];
        {
            const unsigned char* sb = stages;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                fa[0][i] = *reinterpret_cast<const T8*>(sb + a_off + i * 1024);
                fb[0][i] = *reinterpret_cast<const T8*>(sb + b_off + i * 1024);
            }
        }
        for (int ks = 0; ks < nk; ks += 2) {   // (nk is even: K % 256 == 0 on this path)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                issue(ks + s + 3, (buf + 3) & 3);  // the stage consumed in the previous step
                const unsigned char* sb = stages + buf * W2_STAGE_BYTES;
                const unsigned char* sn = stages + ((buf + 1) & 3) * W2_STAGE_BYTES;
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) ga[mi] = *reinterpret_cast<const T8*>(sb + a_off + (4 + mi) * 1024);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) acc[mi][ni] = mfma16(fb[s][ni], fa[s][mi], acc[mi][ni]);
                __builtin_amdgcn_sched_barrier(0);
                // (this wave's reads of the current stage have returned before it passes the barrier: the DMA requests of the next
                //  step overwrite the stage that was current one step earlier)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                dtk_vm_wait<2 * W2_REQ>();  // stage ks + 1 landed; ks + 2 and ks + 3 stay in flight
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 4; ++i) {   // (behind the last step: the repeated last stage, harmless)
                    fa[s ^ 1][i] = *reinterpret_cast<const T8*>(sn + a_off + i * 1024);
                    fb[s ^ 1][i] = *reinterpret_cast<const T8*>(sn + b_off + i * 1024);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) acc[4 + mi][ni] = mfma16(fb[s][ni], ga[mi], acc[4 + mi][ni]);
                __builtin_amdgcn_sched_barrier(0);
                buf = (buf + 1) & 3;
            }
        }
    } else {
    for (int ks = 0; ks < nk; ++ks) {
        issue(ks + 3, (buf + 3) & 3);  // the stage consumed in the previous iteration
        const unsigned char* sb = stages + buf * W2_STAGE_BYTES;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            T8 af[4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                af[mi] = *reinterpret_cast<const T8*>(sb + a_off + (half * 4 + mi) * 1024);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const T8 bfr = *reinterpret_cast<const T8*>(sb + b_off + ni * 1024);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    acc[half * 4 + mi][ni] =
                        mfma16(bfr, af[mi], acc[half * 4 + mi][ni]);   // (W tile) x (token tile)^T: D transposed, see the epilogue
            }
        }
        dtk_vm_wait<2 * W2_REQ>();  // stage ks + 1 landed; ks + 2 and ks + 3 stay in flight
        __syncthreads();
        buf = (buf + 1) & 3;
    }
    }
    dtk_vm_wait<0>();
    // D tiles are TRANSPOSED (the MFMAs above multiply (W tile) x (token tile)^T): lane (fg, fj) holds features 4 fg + r of token fj
    float amax = 0.f;
    if constexpr (EPI == EPI_SWIGLU) {
        // The w12 GEMM of ViT-g (vit_gemm_common.h, swiglu_col): a wave's 64 packed columns are 32 gate columns (fragments ni = 0, 1) and
        // their 32 value columns (ni + 2) -- silu(gate) * value from the lane's own accumulators, staged as the 256 x 128 HIDDEN tile
        // (row pitch 264 B: the 8-byte writes of 16 tokens fall on 16 different bank pairs, as with W2_OPITCH) and written as whole
        // 256-byte rows of out [M][N / 2], 16 bytes per lane, four rows per wave and instruction.
        static_assert(PIPE, "EPI_SWIGLU has no direct-store form");
        constexpr int HP = W2_N + 8;   // staged hidden rows: 128 values x 2 B + 8
        static_assert(W2_M * HP <= W2_LDS_BYTES, "the staged hidden tile must fit");
        __syncthreads();   // every wave's requests have landed (the wait above) and every wave is done with the stages
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int cb = wc * 64 + ni * 16 + fg * 4, hb = wc * 32 + ni * 16 + fg * 4;
            const float4 bg = e.bias ? *reinterpret_cast<const float4*>(e.bias + n0 + cb) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 bv = e.bias ? *reinterpret_cast<const float4*>(e.bias + n0 + cb + 32) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int mi = 0; mi < 8; ++mi) {
                const f4 &g = acc[mi][ni], &v = acc[mi][ni + 2];
                const float h0 = swiglu_pair(g[0] + bg.x, v[0] + bv.x, amax), h1 = swiglu_pair(g[1] + bg.y, v[1] + bv.y, amax);
                const float h2 = swiglu_pair(g[2] + bg.z, v[2] + bv.z, amax), h3 = swiglu_pair(g[3] + bg.w, v[3] + bv.w, amax);
                *reinterpret_cast<T4*>(stages + (wr * 128 + mi * 16 + fj) * HP + hb * 2) = T4{(T)h0, (T)h1, (T)h2, (T)h3};
            }
        }
        __syncthreads();
        const int NH = N >> 1;
        T* const outp = e.out + (n0 >> 1) + (tid & 15) * 8;
#pragma unroll 4
        for (int it = 0; it < W2_M / 32; ++it) {
            const int row = it * 32 + (tid >> 4);
            const uint4 v = staged16(stages + row * HP + (tid & 15) * 16);
            if (m0 + row < M && !DTK_DBG(e.no_store, 4)) *reinterpret_cast<uint4*>(outp + (m0 + row) * NH) = v;
        }
    } else if (PIPE && EPI != EPI_QKV) {
        // Round 6: the [M][N] epilogues leave through LDS.  A store instruction of the direct form below covers 16 tokens x 32 bytes --
        // sixteen quarter lines; with everything but the epilogue switched off (DTK_DEV ablation) the stores of fc1 at D = 1024 ran at
        // 1.5 TB/s and cost a third of the kernel, because a CU holds ONE workgroup of this kernel (128 KB of stages) and nothing
        // overlaps its epilogue.  The stages are dead here: the 256 x 256 tile is staged as 16-bit values (row pitch 520 B) and leaves
        // as whole 512-byte rows, 16 bytes per lane, two rows per wave and instruction.
        __syncthreads();   // every wave's requests have landed (the wait above) and every wave is done with the stages
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int cb = wc * 64 + ni * 16 + fg * 4;
            const float4 b4 = e.bias ? *reinterpret_cast<const float4*>(e.bias + n0 + cb) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 g4 = EPI == EPI_DELTA ? *reinterpret_cast<const float4*>(e.gamma + n0 + cb) : make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll
            for (int mi = 0; mi < 8; ++mi)
                *reinterpret_cast<T4*>(stages + (wr * 128 + mi * 16 + fj) * W2_OPITCH + cb * 2) =
                    gemm_value_tile_t<T, EPI>(acc[mi][ni], b4, g4, amax);
        }
        __syncthreads();
        T* const outp = (EPI == EPI_GELU ? e.out : e.delta) + n0 + (tid & 31) * 8;
#pragma unroll 4
        for (int it = 0; it < W2_M / 16; ++it) {
            const int row = it * 16 + (tid >> 5);
            const uint4 v = staged16(stages + row * W2_OPITCH + (tid & 31) * 16);
            if (m0 + row < M && !DTK_DBG(e.no_store, 4)) *reinterpret_cast<uint4*>(outp + (m0 + row) * N) = v;
        }
    } else if (PIPE && EPI == EPI_QKV && n0 < 2 * e.D) {
        // Q and K tiles the same way (a 256-feature tile is four heads of ONE of q / k / v: D is a multiple of 256 on this path): a
        // token's 64 features of a head are 128 contiguous bytes of q / k [frame][head][position][64].  V^T: the next branch.
        __syncthreads();
        const int which = n0 / e.D, head0 = (n0 - which * e.D) >> 6;
        const float sc = which == 0 ? e.qscale : 1.f;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int cb = wc * 64 + ni * 16 + fg * 4;
            const float4 b4 = e.bias ? *reinterpret_cast<const float4*>(e.bias + n0 + cb) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int mi = 0; mi < 8; ++mi) {
                const f4& a = acc[mi][ni];
                const float v0 = (a[0] + b4.x) * sc, v1 = (a[1] + b4.y) * sc, v2 = (a[2] + b4.z) * sc, v3 = (a[3] + b4.w) * sc;
                if (IsF16<T>::value) amax = amax2(amax2(amax, v0, v1), v2, v3);
                *reinterpret_cast<T4*>(stages + (wr * 128 + mi * 16 + fj) * W2_OPITCH + cb * 2) = T4{(T)v0, (T)v1, (T)v2, (T)v3};
            }
        }
        __syncthreads();
        T* const qk = (which == 0 ? e.q : e.k) + (tid & 7) * 8;
        const int hh = head0 + ((tid & 31) >> 3);
#pragma unroll 4
        for (int it = 0; it < W2_M / 16; ++it) {
            const int row = it * 16 + (tid >> 5);
            const uint4 v = staged16(stages + row * W2_OPITCH + (tid & 31) * 16);
            const long long m = m0 + row;
            if (m < M && !DTK_DBG(e.no_store, 4)) {
                const unsigned f = (unsigned)m / (unsigned)e.S, pos = (unsigned)m - f * (unsigned)e.S;   // (M < 2^31 tokens)
                *reinterpret_cast<uint4*>(qk + (((size_t)f * e.heads + hh) * e.Sp + pos) * 64) = v;
            }
        }
    } else if (PIPE && EPI == EPI_QKV) {
        // V^T tiles: vt[frame][head][feature][position] keeps TOKENS contiguous, so the tile is staged transposed -- sT[feature][token],
        // 16-bit, the same pitch: a lane writes its four features of a token as four 2-byte pieces (the 16 tokens of a piece-write share
        // 8 dwords; the four feature groups of a wave fall on different banks) -- and leaves as 8-byte pieces of four tokens, 64 lanes =
        // 512 contiguous bytes of one feature row, when positions come in fours (S and Sp multiples of 4: 8108 / 8192 at 854 x 476);
        // otherwise (odd test sizes) element by element.  The direct form wrote 2-byte pieces, 16 tokens x 4 rows per instruction, and
        // made a V^T tile's epilogue 2.7 x a Q / K tile's (ViT-L qkv: 39.7 us per tile on average against proj's 34.4).
        __syncthreads();
        const int head0 = (n0 - 2 * e.D) >> 6;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int cb = wc * 64 + ni * 16 + fg * 4;
            const float4 b4 = e.bias ? *reinterpret_cast<const float4*>(e.bias + n0 + cb) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int mi = 0; mi < 8; ++mi) {
                const f4& a = acc[mi][ni];
                const float v[4] = {a[0] + b4.x, a[1] + b4.y, a[2] + b4.z, a[3] + b4.w};
                if (IsF16<T>::value) amax = amax2(amax2(amax, v[0], v[1]), v[2], v[3]);
                unsigned char* sp = stages + cb * W2_OPITCH + (wr * 128 + mi * 16 + fj) * 2;
#pragma unroll
                for (int r = 0; r < 4; ++r) *reinterpret_cast<T*>(sp + r * W2_OPITCH) = (T)v[r];
            }
        }
        __syncthreads();
        if (((e.S | e.Sp) & 3) == 0) {
            const int g = tid & 63;   // tokens 4 g .. 4 g + 3 of the tile: one frame (frames start at multiples of 4), all below M or none
            const long long m = m0 + 4 * g;
            if (m < M && !DTK_DBG(e.no_store, 4)) {
                const unsigned f = (unsigned)m / (unsigned)e.S, pos = (unsigned)m - f * (unsigned)e.S;
                T* const base = e.vt + (((size_t)f * e.heads + head0) * 64) * e.Sp + pos;   // feature c of the tile: + c Sp
#pragma unroll 4
                for (int it = 0; it < W2_N / 8; ++it) {
                    const int c = it * 8 + (tid >> 6);
                    *reinterpret_cast<uint2*>(base + (size_t)c * e.Sp) = *reinterpret_cast<const uint2*>(stages + c * W2_OPITCH + g * 8);
                }
            }
        } else {
            const int t = tid & 255;
            const long long m = m0 + t;
            if (m < M && !DTK_DBG(e.no_store, 4)) {
                const unsigned f = (unsigned)m / (unsigned)e.S, pos = (unsigned)m - f * (unsigned)e.S;
                T* const base = e.vt + (((size_t)f * e.heads + head0) * 64) * e.Sp + pos;
#pragma unroll 4
                for (int it = 0; it < W2_N / 2; ++it) {
                    const int c = it * 2 + (tid >> 8);
                    base[(size_t)c * e.Sp] = *reinterpret_cast<const T*>(stages + c * W2_OPITCH + t * 2);
                }
            }
        }
    } else {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int nb = n0 + wc * 64 + ni * 16 + fg * 4;
#pragma unroll
            for (int mi = 0; mi < 8; ++mi)
                gemm_store_tile_t<T, EPI>(acc[mi][ni], m0 + wr * 128 + mi * 16 + fj, nb, M, N, e, amax);
        }
    }
    amax_report<T, EPI>(amax, e.ovf);
}

}  // namespace
