// vit_gemm_ws.h -- the weight-stationary GEMM of the ViT encoder for K = 384 (QKV, attention projection and fc1 of ViT-S).
#pragma once
#include <type_traits>
#include <utility>
#include "vit_gemm_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// weight-stationary GEMM for K = 384 (QKV, attention projection and fc1 of ViT-S): C[M][N] = A[M][384] . Wt[N][384]^T
//
// A workgroup of four waves owns 256 output features (64 per wave) for a chunk of token tiles; a wave keeps its 64 weight rows in
// registers for the whole chunk (A operand of MFMA 32x32x16: 24 k-steps x 2 row tiles = 192 registers, AGPRs in the V2M = 3 form)
// and the tokens stream through a triple-buffered LDS tile of 32 tokens (24 KB) filled by LDS-DMA two steps ahead, read once per
// wave as the B operand: one ds_read_b128 feeds two MFMAs and there is no K loop with barriers -- one barrier per 32 tokens.
// The weight rows are permuted over the MFMA rows so that in D a lane (token j, half h) holds 16 CONSECUTIVE output
// features (n0 + 32 t + 16 h + r): the epilogue of the previous tile (bias, GELU / Q scale / LayerScale, conversion,
// 16-byte stores) is issued between the MFMAs of the current one.  One workgroup per CU (one wave per SIMD, occupancy 1).
//
// The default form (V2M = 3, HC) cuts that epilogue by hand: a steady-state step is one basic block of 48 MFMAs, each followed by a
// "slot" of the previous tile's epilogue behind a sched_barrier -- 12 slots per group of 8 values in fc1 (the four polynomial chains
// of gelu2 side by side), the flush's four ds_read_b128 behind the first MFMA and its four stores behind the next four, the V^T
// stores one per slot.  Stores are unconditional there: only a wave without columns (n0 >= N, a loop of its own that issues its tile
// requests and joins the barriers) and the globally last token tile (whose epilogue runs behind the loop, predicated) can be out of
// range; the first two steps of a chunk and the tail are peeled.  Bias and LayerScale live in registers, output addresses are a
// base per tile plus a 32-bit lane offset.  docs/KERNELS.md, profiles/gemm_ws_epilogue_isa.md.
// Measured alternatives (all slower on MI355X): staging the outputs through LDS for whole-line stores, one output
// feature per lane (2-byte stores), 4 tokens x 256 B per DMA request, register-staged tiles instead of LDS-DMA.
// ---------------------------------------------------------------------------------------------------------------
constexpr int WS_KS = 24, WS_K = 16 * WS_KS, WS_ROWS = 32, WS_COLS = 256;
constexpr int WS_TILE_BYTES = WS_ROWS * WS_K * 2;
constexpr int WS_LQ = WS_KS / 4;  // LDS-DMA requests per wave per tile
constexpr int WS_PITCH = 144;                    // staging row pitch: 128 B of payload + 16 (conflict-free 16-B accesses)
constexpr int WS_UNIT_BYTES = WS_ROWS * WS_PITCH;  // staging unit: 32 rows x 128 B (64 bf16 or 32 fp32 outputs)

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): the slots of a step as compile-time constants (register arrays are
// indexed by them, which must not depend on a loop being unrolled)
template <class F, int... I>
__device__ __forceinline__ void ws_for_each(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void ws_for_each(F&& f) { ws_for_each(f, std::make_integer_sequence<int, N>{}); }

// ---------------------------------------------------------------------------------------------------------------
// RT = 3 launches: column groups of 384 features on a 1-D grid laid out by a plan.  Group g owns chunks[g] consecutive workgroups,
// each with tpc[g] consecutive token tiles (the last one of a group may be shorter): groups whose epilogue is slower can be given
// more, smaller chunks, so that all workgroups of the one resident round end together.  All groups of fc1 are alike: four times 64;
// qkv gives its V^T group WS96_VT_SHARE chunks and Q and K half of the rest each.
// ---------------------------------------------------------------------------------------------------------------
constexpr int WS96_COLS = 384, WS96_MAX_GROUPS = 4, WS96_WGS = 256;
constexpr int WS96_PITCH = WS96_COLS * 2 + 16;   // staged row of the Q / K tile: 768 B of payload + 16 (gemm_ws_ln_kernel's pitch)
constexpr int WS96_STAGE_BYTES = WS_ROWS * WS96_PITCH;
constexpr int WS96_VT_SHARE = 92;   // chunks of the V^T group of qkv (N = 1152), Q and K get 82 each; 86 would be equal shares
constexpr int WS96_MAX_TPC = 65536;   // token tiles per chunk: 32-bit byte offsets inside a chunk (65536 x 24 KB)
struct Ws96Plan {
    int groups;
    int chunks[WS96_MAX_GROUPS];   // workgroups of group g
    int tpc[WS96_MAX_GROUPS];      // token tiles per chunk of group g
};
// Every tile of every group exactly once; sum of chunks <= 256 (up to 64 x 65536 tiles: beyond that the chunk size stays at its
// 32-bit limit and the grid grows).  Fewer tiles than chunks: one tile per chunk, fewer workgroups.
inline Ws96Plan gemm_ws96_plan(int N, long long rows) {
    Ws96Plan p = {};
    p.groups = N / WS96_COLS;
    const long long tiles = (rows + WS_ROWS - 1) / WS_ROWS;
    // qkv (three groups: Q, K, V^T): the V^T group stores 2-byte values and runs longer per tile, so it gets b > a chunks of fewer tiles:
    // (a, a, b) with 2 a + b <= 256.  b is WS96_VT_SHARE, chosen by the sweep of docs/MEASUREMENTS.md; it depends on N, not on the input.
    int vt_share = WS96_VT_SHARE;
#ifdef DTK_WS96_SWEEP   // (that sweep's build: the share from the environment)
    if (const char* sv = getenv("DTK_WS96_VT_SHARE")) vt_share = atoi(sv);
#endif
    for (int g = 0; g < p.groups; ++g) {
        const int share = p.groups != 3 ? WS96_WGS / p.groups : g == 2 ? vt_share : (WS96_WGS - vt_share) / 2;
        long long tpc = (tiles + share - 1) / share;
        if (tpc < 1) tpc = 1;
        if (tpc > WS96_MAX_TPC) tpc = WS96_MAX_TPC;
        p.tpc[g] = (int)tpc;
        p.chunks[g] = (int)((tiles + tpc - 1) / tpc);
    }
    return p;
}
constexpr bool gemm_ws96_role(int epi) { return epi == EPI_GELU || epi == EPI_QKV; }   // the epilogues that have this form
inline bool gemm_ws96_fits(int N) { return N % WS96_COLS == 0 && N / WS96_COLS >= 1 && N / WS96_COLS <= WS96_MAX_GROUPS; }
inline dim3 gemm_ws96_grid(const Ws96Plan& p) {
    unsigned n = 0;
    for (int g = 0; g < p.groups; ++g) n += (unsigned)p.chunks[g];
    return dim3(n);
}
// What a workgroup owns.  RT = 2: the launch's last argument is the tiles per chunk, blockIdx.x the column group, blockIdx.y the chunk.
// RT = 3: the argument is the plan, blockIdx.x counts the chunks of group 0, then those of group 1, ...
struct WsWhere {
    unsigned colgroup;
    int tpc;
    unsigned chunk;   // the workgroup's first token tile is chunk * tpc
};
template <int RT> struct WsArg { typedef int type; };
template <> struct WsArg<3> { typedef Ws96Plan type; };
__device__ __forceinline__ WsWhere ws_where(int tiles_per_chunk) {
    return {blockIdx.x, tiles_per_chunk, blockIdx.y};
}
__device__ __forceinline__ WsWhere ws_where(const Ws96Plan& plan) {
    // (constant indices into the plan: a variable one would move the kernel argument into scratch memory)
    int c = blockIdx.x, g = 0, tpc = plan.tpc[0], first = 0;
#pragma unroll
    for (int i = 0; i + 1 < WS96_MAX_GROUPS; ++i) {
        first += plan.chunks[i];
        if (i + 1 < plan.groups && (int)blockIdx.x >= first) { g = i + 1; c = (int)blockIdx.x - first; tpc = plan.tpc[i + 1]; }
    }
    return {(unsigned)g, tpc, (unsigned)c};
}

// V2M (round 4, default 3): bit 0 = weights in AGPRs (loaded there by asm; the builtin MFMA takes them from there as they are)
// and zero accumulators through the MFMA's C operand; bit 1 = token tiles by LDS-DMA through a buffer descriptor (scalar tile
// offset + constant per-lane offset: 3 issue slots per request instead of ~13).  V2M = 0 is the round 1-3 form, kept for the
// A / B measurement (DTK_VIT_GEMM_WS_V1).  Same-box A / B: proj 4.97 -> 3.62 ms, qkv 12.34 -> 12.10, fc1 14.68 -> 14.55 ms per step.
// HC (default with V2M = 3): the hand-cut step described above; <T, EPI, 3, false> is the form before it (DTK_DEV bit 128, and any
// N that is not a multiple of 64).  V2M = 0 shares none of the hand-cut code: it is the bitwise reference of
// tests/test_gpu_vit_gemm_ws_epilogue.py.
//
// RT: 32-row weight tiles per wave.  RT = 2 is the form described so far.  RT = 3 (hand-cut form only, fc1 and qkv) gives a wave 96
// features and a workgroup 384: the same token tile, fetch, barrier and fragment reads serve 72 MFMAs instead of 48 -- one
// ds_read_b128 feeds three -- and every output is still the same chain of 24 MFMAs, so the bits do not change.  288 weight registers,
// 240 of them AGPRs (as in gemm_ws_ln_kernel); the bias of a group of eight values comes from the s_bias table in the group's first
// slot instead of living in registers.  qkv at RT = 3: column group g is q, k or v, so a workgroup is all-Q, all-K or all-V^T; Q / K
// stage the workgroup's [32][384] tile in LDS (double-buffered) and flush it as whole 128-byte (token, head) lines behind the barrier
// that completes it, six ds_read_b128 behind the first MFMA of the next step and six stores behind the following ones; V^T stores one
// 2-byte value per slot in slots 0 .. 47.
template <typename T, int EPI, int V2M = 3, bool HC = (V2M == 3), int RT = 2>
__global__ __launch_bounds__(256) void gemm_ws_kernel(const T* __restrict__ A, const T* __restrict__ Wt,
                                                      long long M, int N, GemmEpi<T> e, typename WsArg<RT>::type where) {
    typedef typename Vec<T>::t8 T8;
    typedef typename Vec<T>::t4 T4;
    (void)sizeof(T8); (void)sizeof(T4);
    constexpr bool V2 = (V2M & 1) != 0;       // AGPR weights + zero C operand
    constexpr bool V2D = (V2M & 2) != 0;      // descriptor LDS-DMA
    static_assert(!HC || V2M == 3, "the hand-cut step is built on the AGPR weights and the descriptor LDS-DMA");
    static_assert(RT == 2 || (RT == 3 && HC && (EPI == EPI_GELU || EPI == EPI_QKV)), "96 features per wave: the hand-cut fc1 and qkv steps only");
    constexpr int WCOLS = 32 * RT;                  // features per wave
    constexpr int AGPR_FRAGS = RT == 2 ? 2 * WS_KS : 60;   // weight fragments pinned to AGPRs by asm (RT = 3: 240 of the 256, of 72)
    operand_mode<T>();
    __shared__ __attribute__((aligned(1024))) unsigned char toks[3][WS_TILE_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char stage[4][2][WS_UNIT_BYTES];  // per wave: two staging units
    // RT = 3, Q / K: the workgroup's [32][384] 16-bit tile, padded pitch, double-buffered (a wave's 96 features are one and a half heads)
    constexpr bool STG3 = RT == 3 && EPI == EPI_QKV;
    __shared__ __attribute__((aligned(16))) unsigned char stage3[STG3 ? 2 : 1][STG3 ? WS96_STAGE_BYTES : 16];
    __shared__ __attribute__((aligned(16))) float s_bias[4][WCOLS], s_gamma[4][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const WsWhere wh = ws_where(where);
    const int tiles_per_chunk = wh.tpc;
    const int n0 = wh.colgroup * (4 * WCOLS) + w * WCOLS;
    const long long total_tiles = (M + WS_ROWS - 1) / WS_ROWS;
    const long long tile0 = (long long)wh.chunk * tiles_per_chunk;
    if (tile0 >= total_tiles) return;
    const int NT = (int)((total_tiles - tile0) < tiles_per_chunk ? (total_tiles - tile0) : tiles_per_chunk);
    // weights: MFMA row i of row tile t carries output feature n0 + 32 t + nl(i), nl chosen so that D row
    // (r & 3) + 8 (r >> 2) + 4 h  <->  feature 16 h + r
    const int nl = (j & 3) + 4 * (j >> 3) + 16 * ((j >> 2) & 1);
    T8 wf[RT][WS_KS];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int row = min(n0 + t * 32 + nl, N - 1);
        const T* wp = Wt + (size_t)row * WS_K + h * 8;
#pragma unroll
        for (int ks = 0; ks < WS_KS; ++ks) {
            if (V2 && t * WS_KS + ks < AGPR_FRAGS) asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(wf[t][ks]) : "v"(wp + ks * 16) : "memory");
            else wf[t][ks] = *reinterpret_cast<const T8*>(wp + ks * 16);
        }
    }
    if (V2) {
        // the loads above are invisible to the compiler's own vmcnt bookkeeping: wait, then re-define every loaded register behind
        // the wait (an empty volatile asm with a "+a" operand emits nothing, but volatile asms keep their order and no use of
        // wf can be scheduled above its re-definition -- ADVICE r4: before, only scheduling luck kept uses behind the wait)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int ks = 0; ks < WS_KS; ++ks)
                if (t * WS_KS + ks < AGPR_FRAGS) asm volatile("" : "+a"(wf[t][ks]));
    }
    if constexpr (!HC) {
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
    float amax = 0.f;
    // (DTK_DEV ablations, both forms: no_store & 32 = no stores, the values folded into `dbg_sink` so that the arithmetic stays;
    //  & 64 = bias + convert only, stores kept.  The older & 3 clears `ok`, which skips the arithmetic sunk behind it as well.)
    unsigned dbg_sink = 0;
    auto dbg_fold = [&](const auto& val) {
        unsigned b[sizeof(val) / 4];
        __builtin_memcpy(b, &val, sizeof(val));
#pragma unroll
        for (unsigned i = 0; i < sizeof(val) / 4; ++i) dbg_sink |= b[i];
    };
    if constexpr (HC) {
        // ------------------------------------------------------------------------------------------------------
        // The hand-cut form.  Stores can only be out of range in a wave whose columns lie past N (constant for the launch) and in
        // the globally last token tile, whose epilogue always runs BEHIND the loop: so idle waves get a loop of their own, the
        // first two steps of a chunk and the tail are peeled, and a steady-state step is one basic block -- 48 MFMAs, each
        // followed by one slice ("slot") of the previous tile's epilogue behind a sched_barrier, stores unconditional.
        // ------------------------------------------------------------------------------------------------------
        typedef std::integral_constant<bool, true> Yes;
        typedef std::integral_constant<bool, false> No;
        if (n0 >= N) {   // idle wave (last column group of N = 1152 / 384): its share of the tile requests and the barriers, nothing else
            issue(0, 0);
            issue(min(1, NT - 1), 1);
            dtk_vm_wait<WS_LQ>();
            __syncthreads();
            int b0 = 0;
            for (int n = 0; n + 1 < NT; n += 2) {
                const int b1 = b0 == 2 ? 0 : b0 + 1, b2 = b1 == 2 ? 0 : b1 + 1;
                issue(min(n + 2, NT - 1), b2);
                dtk_vm_wait<WS_LQ>();
                __syncthreads();
                issue(min(n + 3, NT - 1), b0);
                dtk_vm_wait<WS_LQ>();
                __syncthreads();
                b0 = b2;
            }
            dtk_vm_wait<0>();
            return;
        }
        // bias (and LayerScale) of this lane's 2 x 16 features: registers for the whole chunk (the launcher gives this form whole
        // 64-column waves only: N % 64 == 0)
        float bia[2][16], gam[2][16];
        if constexpr (RT == 2) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int nf = n0 + 32 * t + 16 * h + r;
                    bia[t][r] = e.bias ? e.bias[nf] : 0.f;
                    gam[t][r] = (EPI == EPI_DELTA) ? e.gamma[nf] : 1.f;
                }
        } else {
            // RT = 3: 3 x 16 bias registers do not fit beside the GELU chains.  The wave's 96 values go into its row of s_bias (read
            // back by this wave only, eight at a time, in the first slot of each group of eight values; `sb` in the slots is the lane's base there).
            (void)bia; (void)gam;
            for (int i = lane; i < WCOLS; i += 64) s_bias[w][i] = e.bias ? e.bias[n0 + i] : 0.f;
        }
        const bool dbg_nost = DTK_DBG(e.no_store, 3) || DTK_DBG(e.no_store, 32);   // DTK_DEV: no stores (32: the arithmetic stays live)
        const bool dbg_noar = DTK_DBG(e.no_store, 64);                              // DTK_DEV: bias + convert only, stores kept
        auto run = [&](auto vt_tag) {
            constexpr bool VT = decltype(vt_tag)::value;     // a V^T wave of the QKV GEMM (which == 2)
            constexpr bool STG = EPI != EPI_GELU && !VT;     // outputs leave as whole lines through the staging unit
            const long long mt0 = tile0 * WS_ROWS;
            // Output addresses: a base per tile that moves by an increment, plus 32-bit lane offsets; no multiply per store.
            //   GELU   per-lane pointer to (token j, feature n0 + 16 h) of the epilogue's tile
            //   DELTA  uniform pointer to (first token, n0) of the staged tile; lane offset (row, piece)
            //   Q / K  uniform pointer to (frame, head, position of the first token) of the staged tile; a lane whose row lies behind the
            //          frame end adds `cross` (a tile crosses at most one frame end: launch_gemm, ws_fits)
            //   V^T    the same for the epilogue's tile, tokens along the fastest axis
            T* op = nullptr;
            T* up = nullptr;
            int s0 = 0;
            unsigned cross = 0;
            if constexpr (EPI == EPI_GELU) op = e.out + (mt0 + j) * N + n0 + 16 * h;
            if constexpr (EPI == EPI_DELTA) up = e.delta + mt0 * N + n0;
            if constexpr (EPI == EPI_QKV) {
                const int f0 = (int)(mt0 / e.S);
                s0 = (int)(mt0 - (long long)f0 * e.S);
                if (VT) {
                    up = e.vt + (((size_t)f0 * e.heads + head) * 64) * e.Sp + s0;
                    cross = (unsigned)(e.heads * 64 * e.Sp - e.S);
                } else {
                    up = (which == 0 ? e.q : e.k) + (((size_t)f0 * e.heads + head) * e.Sp + s0) * 64;
                    cross = (unsigned)((e.heads * e.Sp - e.S) * 64);
                }
                if constexpr (RT == 3) {
                    // the workgroup is all-Q, all-K or all-V^T.  V^T rows (head, dh) are the wave's features 96 w ..; Q / K start at head 0
                    if (VT) up = e.vt + ((size_t)f0 * e.heads * 64 + (n0 - which * e.D)) * e.Sp + s0;
                    else up = (which == 0 ? e.q : e.k) + ((size_t)f0 * e.heads * e.Sp + s0) * 64;
                }
            }
            const size_t out_step = (size_t)WS_ROWS * N;
            unsigned char* const sw = &stage[w][0][0] + j * WS_PITCH + 32 * h;                         // staging: this lane's 16 features of token j
            const unsigned char* const sr = &stage[w][0][0] + (lane >> 3) * WS_PITCH + (lane & 7) * 16;  // flush: row lane / 8 (+ 8 p), piece lane % 8
            auto next_tile = [&]() {   // the output base moves on by one token tile
                if constexpr (EPI == EPI_GELU) op += out_step;
                if constexpr (EPI == EPI_DELTA) up += out_step;
                if constexpr (EPI == EPI_QKV) {
                    s0 += WS_ROWS;
                    up += VT ? WS_ROWS : WS_ROWS * 64;
                    if (s0 >= e.S) { s0 -= e.S; up += cross; }
                }
            };
            auto st16 = [&](T* p, unsigned off, dtk_u4 val, bool ok) {   // 16 bytes to p + off elements
                if (!dbg_nost) { if (ok) *reinterpret_cast<dtk_u4*>(p + off) = val; }
                else dbg_fold(val);
            };
            // ---- the epilogue of one tile in 48 slots; PRED: stores of rows < valid only (the tail), FL: with the flush of the tile before
            float v[8];
            f2 sx[4], uu[4], pp[4];
            T8 o;
            constexpr int NFL = STG3 ? 6 : 4;   // flush pieces per lane and tile
            dtk_u4 fv[NFL];
            unsigned voff = 0;
            // RT = 3 Q / K: `sto` = byte offset of the staging buffer this step's epilogue writes (0: tiles in accA, WS96_STAGE_BYTES: accB); the
            // flush reads the other one.  Lane (row tid / 8, piece lane % 8) flushes that row's 128-byte line of head p, p = 0 .. 5.
            unsigned sto = 0, flo = 0;
            unsigned char* const sw3 = STG3 ? &stage3[0][0] + j * WS96_PITCH + (w * WCOLS + 16 * h) * 2 : nullptr;
            const unsigned char* const sr3 = STG3 ? &stage3[0][0] + (tid >> 3) * WS96_PITCH + (lane & 7) * 16 : nullptr;
            constexpr float GC[9] = {1.112979639e-10f, -1.065557687e-08f, 4.510875158e-07f, -1.125288873e-05f, 1.868377149e-04f,
                                     -2.217123518e-03f, 1.963194646e-02f, -1.326889843e-01f, 7.978046536e-01f};   // gelu2
            auto flush_reads = [&]() {
                ws_for_each<NFL>([&](auto p_tag) {
                    constexpr int p = decltype(p_tag)::value;
                    if constexpr (STG3) fv[p] = *reinterpret_cast<const dtk_u4*>(sr3 + flo + 128 * p);
                    else fv[p] = *reinterpret_cast<const dtk_u4*>(sr + 8 * p * WS_PITCH);
                });
            };
            auto flush_store = [&](auto pred_tag, auto p_tag, int valid) {
                constexpr int p = decltype(p_tag)::value;
                if constexpr (STG3) {
                    const int row3 = tid >> 3;
                    const bool ok3 = decltype(pred_tag)::value ? row3 < valid : true;
                    st16(up, (unsigned)(row3 * 64 + (lane & 7) * 8 + p * e.Sp * 64) + (s0 + row3 >= e.S ? cross : 0u), fv[p], ok3);
                    return;
                }
                const int row = 8 * p + (lane >> 3);
                const bool ok = decltype(pred_tag)::value ? row < valid : true;
                if constexpr (EPI == EPI_DELTA) st16(up, (unsigned)(row * N + (lane & 7) * 8), fv[p], ok);
                else st16(up, (unsigned)(row * 64 + (lane & 7) * 8) + (s0 + row >= e.S ? cross : 0u), fv[p], ok);
            };
            float4 bi0, bi1, bj0, bj1;   // RT = 3: the bias of the group of eight values in flight (V^T: two sets, the next group's on its way)
            auto slot = [&](auto pred_tag, auto fl_tag, const f16v (&acc)[RT], auto s_tag, int valid) {
                constexpr bool PRED = decltype(pred_tag)::value, FL = decltype(fl_tag)::value;
                constexpr int s = decltype(s_tag)::value;
                const bool ok = PRED ? j < valid : true;
                if constexpr (EPI == EPI_GELU && RT == 3) {
                    const float* const sb = &s_bias[w][16 * h];
                    // six groups of eight values, 12 slots each: the RT = 2 schedule one slot later, its free last slot taken by the
                    // bias read in front (the read's latency passes under the MFMA between slots 0 and 1)
                    constexpr int u = s / 12, ph = s % 12, t = u >> 1, hv = u & 1;
                    if (ph == 0) {
                        bi0 = *reinterpret_cast<const float4*>(sb + 32 * t + 8 * hv);
                        bi1 = *reinterpret_cast<const float4*>(sb + 32 * t + 8 * hv + 4);
                    } else if (ph <= 2) {
                        const float4 bq = ph == 1 ? bi0 : bi1;
                        const float bb[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
                        for (int r = 4 * (ph - 1); r < 4 * (ph - 1) + 4; ++r) v[r] = acc[t][8 * hv + r] + bb[r & 3];
                        if (IsF16<T>::value) {   // the stored GELU(v): the positive part of v
#pragma unroll
                            for (int r = 4 * (ph - 1); r < 4 * (ph - 1) + 4; r += 2) amax = fmaxf(fmaxf(amax, v[r]), v[r + 1]);
                        }
                    }
                    if (dbg_noar) {
                        if (ph == 10) {
#pragma unroll
                            for (int r = 0; r < 8; ++r) o[r] = (T)v[r];
                        }
                    } else if (ph == 3) {   // gelu2, its four chains side by side
                        const f2 c = {4.25f, 4.25f};
#pragma unroll
                        for (int q = 0; q < 4; ++q) sx[q] = __builtin_elementwise_min(__builtin_elementwise_max(f2{v[2 * q], v[2 * q + 1]}, -c), c);
#pragma unroll
                        for (int q = 0; q < 4; ++q) uu[q] = sx[q] * sx[q];
                    } else if (ph >= 4 && ph <= 7) {
#pragma unroll
                        for (int l = 2 * (ph - 4); l < 2 * (ph - 4) + 2; ++l)
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                pp[q] = __builtin_elementwise_fma(l == 0 ? f2{GC[0], GC[0]} : pp[q], uu[q], f2{GC[l + 1], GC[l + 1]});
                    } else if (ph == 8) {
                        const f2 one = {1.f, 1.f};
#pragma unroll
                        for (int q = 0; q < 4; ++q) pp[q] = __builtin_elementwise_min(__builtin_elementwise_max(sx[q] * pp[q], -one), one);
                    } else if (ph == 9) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const f2 hx = f2{v[2 * q], v[2 * q + 1]} * f2{0.5f, 0.5f};
                            uu[q] = __builtin_elementwise_fma(hx, pp[q], hx);
                        }
                    } else if (ph == 10) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) { o[2 * q] = (T)uu[q][0]; o[2 * q + 1] = (T)uu[q][1]; }
                    }
                    if (ph == 11) st16(op, (unsigned)(32 * t + 8 * hv), __builtin_bit_cast(dtk_u4, o), ok);
                } else if constexpr (EPI == EPI_GELU) {
                    constexpr int u = s / 12, ph = s % 12, t = u >> 1, hv = u & 1;
                    if (ph < 2) {
#pragma unroll
                        for (int r = 4 * ph; r < 4 * ph + 4; ++r) v[r] = acc[t][8 * hv + r] + bia[t][8 * hv + r];
                        if (IsF16<T>::value) {   // the stored GELU(v): the positive part of v
#pragma unroll
                            for (int r = 4 * ph; r < 4 * ph + 4; r += 2) amax = fmaxf(fmaxf(amax, v[r]), v[r + 1]);
                        }
                    }
                    if (dbg_noar) {
                        if (ph == 9) {
#pragma unroll
                            for (int r = 0; r < 8; ++r) o[r] = (T)v[r];
                        }
                    } else if (ph == 2) {   // gelu2, its four chains side by side
                        const f2 c = {4.25f, 4.25f};
#pragma unroll
                        for (int q = 0; q < 4; ++q) sx[q] = __builtin_elementwise_min(__builtin_elementwise_max(f2{v[2 * q], v[2 * q + 1]}, -c), c);
#pragma unroll
                        for (int q = 0; q < 4; ++q) uu[q] = sx[q] * sx[q];
                    } else if (ph >= 3 && ph <= 6) {
#pragma unroll
                        for (int l = 2 * (ph - 3); l < 2 * (ph - 3) + 2; ++l)
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                pp[q] = __builtin_elementwise_fma(l == 0 ? f2{GC[0], GC[0]} : pp[q], uu[q], f2{GC[l + 1], GC[l + 1]});
                    } else if (ph == 7) {
                        const f2 one = {1.f, 1.f};
#pragma unroll
                        for (int q = 0; q < 4; ++q) pp[q] = __builtin_elementwise_min(__builtin_elementwise_max(sx[q] * pp[q], -one), one);
                    } else if (ph == 8) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const f2 hx = f2{v[2 * q], v[2 * q + 1]} * f2{0.5f, 0.5f};
                            uu[q] = __builtin_elementwise_fma(hx, pp[q], hx);
                        }
                    } else if (ph == 9) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) { o[2 * q] = (T)uu[q][0]; o[2 * q + 1] = (T)uu[q][1]; }
                    }
                    if (ph == 10) {
                        // (staged for whole-line stores like q / k / delta, on top of this flush: fc1 14.73 against 14.47 ms per step, same
                        //  session -- the 16-byte pieces stay; docs/NEGATIVE_RESULTS.md)
                        st16(op, (unsigned)(32 * t + 8 * hv), __builtin_bit_cast(dtk_u4, o), ok);
                    }
                } else if constexpr (STG3 && STG) {
                    const float* const sb = &s_bias[w][16 * h];
                    // Q / K at RT = 3: the RT = 2 schedule of a group of eight values (a pair every other slot, one ds_write_b128 in slot 9)
                    // into the workgroup's tile; the group's bias from s_bias in slot 0; six flush pieces behind the first MFMA
                    if constexpr (FL && s == 0) flush_reads();
                    if constexpr (FL && s >= 1 && s <= NFL) flush_store(No{}, std::integral_constant<int, s - 1>{}, WS_ROWS);
                    constexpr int u = s / 12, ph = s % 12, t = u >> 1, hv = u & 1;
                    if constexpr (ph == 0) {
                        bi0 = *reinterpret_cast<const float4*>(sb + 32 * t + 8 * hv);
                        bi1 = *reinterpret_cast<const float4*>(sb + 32 * t + 8 * hv + 4);
                    } else if constexpr ((ph & 1) && ph < 9) {
                        constexpr int r0 = (ph - 1) & 7, r1 = ph & 7;   // this slot's pair of values
                        const float bb[8] = {bi0.x, bi0.y, bi0.z, bi0.w, bi1.x, bi1.y, bi1.z, bi1.w};
                        const float v0 = acc[t][8 * hv + r0] + bb[r0], v1 = acc[t][8 * hv + r1] + bb[r1];
                        if (IsF16<T>::value && !dbg_noar) amax = amax2(amax, v0 * qsc, v1 * qsc);
                        if (dbg_noar) { o[r0] = (T)v0; o[r1] = (T)v1; }
                        else { o[r0] = (T)(v0 * qsc); o[r1] = (T)(v1 * qsc); }
                    } else if constexpr (ph == 9) {
                        *reinterpret_cast<T8*>(sw3 + sto + 64 * t + 16 * hv) = o;
                    }
                } else if constexpr (STG3) {
                    const float* const sb = &s_bias[w][16 * h];
                    // V^T at RT = 3: 48 values, one 2-byte store per slot in slots 0 .. 47; row (head, dh) = the wave's feature.  The bias of
                    // group u + 1 is read in slot 3 of group u (group 0: in slot 0) into the other of two register sets
                    if constexpr (s == 0) {
                        voff = (unsigned)(16 * h * e.Sp + j) + (s0 + j >= e.S ? cross : 0u);
                        bi0 = *reinterpret_cast<const float4*>(sb);
                        bi1 = *reinterpret_cast<const float4*>(sb + 4);
                    }
                    if constexpr (s < 16 * RT) {
                        constexpr int u = s / 8, r = s % 8, t = u >> 1, hv = u & 1;
                        if constexpr (r == 3 && u + 1 < 2 * RT) {
                            constexpr int tn = (u + 1) >> 1, hn = (u + 1) & 1;
                            if constexpr (u & 1) {
                                bi0 = *reinterpret_cast<const float4*>(sb + 32 * tn + 8 * hn);
                                bi1 = *reinterpret_cast<const float4*>(sb + 32 * tn + 8 * hn + 4);
                            } else {
                                bj0 = *reinterpret_cast<const float4*>(sb + 32 * tn + 8 * hn);
                                bj1 = *reinterpret_cast<const float4*>(sb + 32 * tn + 8 * hn + 4);
                            }
                        }
                        const float4 q0 = (u & 1) ? bj0 : bi0, q1 = (u & 1) ? bj1 : bi1;
                        const float bb[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                        v[r] = acc[t][8 * hv + r] + bb[r];
                        if (IsF16<T>::value && (r & 1) && !dbg_noar) amax = amax2(amax, v[r - 1] * qsc, v[r] * qsc);
                        const T val = (T)v[r];
                        T* const p = up + (size_t)(32 * t + 8 * hv + r) * e.Sp;
                        if (!dbg_nost) { if (ok) p[voff] = val; }
                        else dbg_fold(typename Vec<T>::t2{val, val});
                    }
                } else if constexpr (STG) {
                    if constexpr (FL && s == 0) flush_reads();
                    if constexpr (FL && s >= 1 && s <= 4) flush_store(No{}, std::integral_constant<int, s - 1>{}, WS_ROWS);
                    constexpr int u = s / 12, ph = s % 12, t = u >> 1, hv = u & 1;
                    if (ph & 1) {
                        if (ph < 9) {
                            constexpr int r0 = (ph - 1) & 7, r1 = ph & 7;   // this slot's pair of values
                            const float v0 = acc[t][8 * hv + r0] + bia[t][8 * hv + r0], v1 = acc[t][8 * hv + r1] + bia[t][8 * hv + r1];
                            if (EPI == EPI_QKV && IsF16<T>::value && !dbg_noar) amax = amax2(amax, v0 * qsc, v1 * qsc);
                            if (dbg_noar) { o[r0] = (T)v0; o[r1] = (T)v1; }
                            else if (EPI == EPI_DELTA) { o[r0] = (T)(v0 * gam[t][8 * hv + r0]); o[r1] = (T)(v1 * gam[t][8 * hv + r1]); }
                            else { o[r0] = (T)(v0 * qsc); o[r1] = (T)(v1 * qsc); }
                        } else if (ph == 9) {
                            *reinterpret_cast<T8*>(sw + 64 * t + 16 * hv) = o;
                        }
                    }
                } else {   // V^T[f][head][dh][s]: consecutive lanes are consecutive tokens; 2-byte stores, one per slot
                    if (s == 0) voff = (unsigned)(16 * h * e.Sp + j) + (s0 + j >= e.S ? cross : 0u);
                    if (s < 32) {
                        constexpr int u = (s & 31) / 8, r = s % 8, t = u >> 1, hv = u & 1;
                        v[r] = acc[t][8 * hv + r] + bia[t][8 * hv + r];
                        if (IsF16<T>::value && (r & 1) && !dbg_noar) amax = amax2(amax, v[r - 1] * qsc, v[r] * qsc);
                        const T val = (T)v[r];
                        T* const p = up + (size_t)(32 * t + 8 * hv + r) * e.Sp;
                        if (!dbg_nost) { if (ok) p[voff] = val; }
                        else dbg_fold(typename Vec<T>::t2{val, val});
                    }
                }
            };
            auto tail_epi = [&](const f16v (&acc)[RT], int valid) {
                ws_for_each<RT * WS_KS>([&](auto s_tag) { slot(Yes{}, No{}, acc, s_tag, valid); });
                if (!STG) next_tile();
            };
            auto tail_flush = [&](int valid) {
                if constexpr (STG) {
                    flush_reads();
                    ws_for_each<NFL>([&](auto p_tag) { flush_store(Yes{}, p_tag, valid); });
                    next_tile();
                }
            };
            // one step: the MFMAs of the tile in `buf` into accN; PREV: behind each, a slot of the previous tile's epilogue (accP)
            auto step = [&](auto prev_tag, auto fl_tag, int buf, f16v (&accN)[RT], const f16v (&accP)[RT]) {
                constexpr bool PREV = decltype(prev_tag)::value, FL = decltype(fl_tag)::value;
                const unsigned char* base = &toks[0][0] + buf * WS_TILE_BYTES;
                const f16v zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // inline constant C
                T8 b[3];
                b[0] = *reinterpret_cast<const T8*>(base + frag_off[0]);
                b[1] = *reinterpret_cast<const T8*>(base + frag_off[1]);
                ws_for_each<RT * WS_KS>([&](auto s_tag) {
                    constexpr int ks = decltype(s_tag)::value / RT, t = decltype(s_tag)::value % RT;
                    if constexpr (t == 0 && ks + 2 < WS_KS)
                        b[(ks + 2) % 3] = *reinterpret_cast<const T8*>(base + frag_off[(ks + 2) & 7] + ((ks + 2) >> 3) * 1024);
                    // (the builtin, not an asm MFMA: see the V2M = 0 .. 3 step below)
                    accN[t] = mfma32(wf[t][ks], b[ks % 3], ks == 0 ? zero16 : accN[t]);
                    if constexpr (PREV) {
                        __builtin_amdgcn_sched_barrier(0);
                        slot(No{}, fl_tag, accP, s_tag, WS_ROWS);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                });
                // (staged forms: `up` follows the FLUSHED tile, two behind; the others the epilogue's tile, one behind)
                if (STG ? FL : PREV) next_tile();
            };
            f16v accA[RT], accB[RT];
            issue(0, 0);
            issue(min(1, NT - 1), 1);
            dtk_vm_wait<WS_LQ>();
            __syncthreads();
            int n = 0, b0 = 0;
            auto pair = [&](auto first_tag) {
                constexpr bool FIRST = decltype(first_tag)::value;
                const int b1 = b0 == 2 ? 0 : b0 + 1, b2 = b1 == 2 ? 0 : b1 + 1;
                issue(min(n + 2, NT - 1), b2);
                if constexpr (STG3) { sto = WS96_STAGE_BYTES; flo = 0; }   // (epilogue of a tile in accB, flush of the accA tile before it)
                if (FIRST) step(No{}, No{}, b0, accA, accB);
                else step(Yes{}, Yes{}, b0, accA, accB);
                dtk_vm_wait<WS_LQ>();
                __syncthreads();
                issue(min(n + 3, NT - 1), b0);
                if constexpr (STG3) { sto = 0; flo = WS96_STAGE_BYTES; }
                if (FIRST) step(Yes{}, No{}, b1, accB, accA);
                else step(Yes{}, Yes{}, b1, accB, accA);
                dtk_vm_wait<WS_LQ>();
                __syncthreads();
                b0 = b2;
                n += 2;
            };
            if (NT >= 2) pair(Yes{});
            while (n + 1 < NT) pair(No{});
            const long long left = M - (tile0 + NT - 1) * WS_ROWS;   // valid rows of the chunk's last tile
            const int valid = left < WS_ROWS ? (int)left : WS_ROWS;
            const bool odd = n < NT;  // one more tile
            if (odd) {
                if constexpr (STG3) { sto = WS96_STAGE_BYTES; flo = 0; }
                if (n > 0) step(Yes{}, Yes{}, b0, accA, accB);
                else step(No{}, No{}, b0, accA, accB);
            }
            if constexpr (STG3 && STG) {
                // the staging tile is the workgroup's: the tile staged in an odd last step is complete, and every wave's flush reads of the
                // other buffer are done, only behind a barrier; the last tile then goes into the buffer its accumulators' parity names
                __syncthreads();
                flo = odd ? WS96_STAGE_BYTES : 0;
                sto = odd ? 0 : WS96_STAGE_BYTES;
            }
            if (NT > 1) tail_flush(WS_ROWS);
            // (the last tile's accumulators by VALUE: two calls of the tail on accA / accB are merged into one on a pointer, which
            //  takes both arrays out of the registers for the whole kernel)
            if constexpr (RT == 2) {
                const f16v accL[2] = {odd ? accA[0] : accB[0], odd ? accA[1] : accB[1]};
                tail_epi(accL, valid);
            } else {
                const f16v accL[3] = {odd ? accA[0] : accB[0], odd ? accA[1] : accB[1], odd ? accA[2] : accB[2]};
                tail_epi(accL, valid);
            }
            if constexpr (STG3 && STG) {
                __syncthreads();
                flo = sto;
            }
            tail_flush(valid);
        };
        if constexpr (EPI == EPI_QKV) {
            if (which == 2) run(Yes{});
            else run(No{});
        } else {
            run(No{});
        }
        if (DTK_DBG(e.no_store, 32) && dbg_sink == 0x9e3779b9u) amax = 65504.f;   // (DTK_DEV: keeps the values of disabled stores live)
        amax_report<T, EPI>(amax, e.ovf);
        dtk_vm_wait<0>();
        return;
    }
    // epilogue of 8 values (row tile t, half hv of this lane's 16 features): features nb .. nb + 7
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
                else if (!DTK_DBG(e.no_store, 64)) amax = amax2(amax, v[r] * qsc, v[r + 1] * qsc);
            }
        }
        if (EPI == EPI_GELU) {
            T8 o;
#pragma unroll
            for (int r = 0; r < 8; r += 2) {
                const f2 g = DTK_DBG(e.no_store, 64) ? f2{v[r], v[r + 1]} : gelu2(f2{v[r], v[r + 1]});
                o[r] = (T)g[0];
                o[r + 1] = (T)g[1];
            }
            // (staging the GELU output for whole-line stores measured slower than these scattered 16-byte stores)
            if (DTK_DBG(e.no_store, 32)) dbg_fold(o);
            else if (ok) *reinterpret_cast<T8*>(e.out + m_ep * N + nb) = o;
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
                if (DTK_DBG(e.no_store, 32)) {
#pragma unroll
                    for (int r = 0; r < 8; r += 2) dbg_fold(typename Vec<T>::t2{(T)v[r], (T)v[r + 1]});
                } else if (ok) {
                    T* vp = e.vt + (((size_t)f_ep * e.heads + head) * 64 + dh) * e.Sp + s_ep;
#pragma unroll
                    for (int r = 0; r < 8; ++r) vp[(size_t)r * e.Sp] = (T)v[r];
                }
            } else {
                T8 o;
#pragma unroll
                for (int r = 0; r < 8; ++r) o[r] = DTK_DBG(e.no_store, 64) ? (T)v[r] : (T)(v[r] * qsc);
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
                    if (DTK_DBG(e.no_store, 32)) dbg_fold(val);
                    else if (mt_fl + row < M) {
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
    if (DTK_DBG(e.no_store, 32) && dbg_sink == 0x9e3779b9u) amax = 65504.f;
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
