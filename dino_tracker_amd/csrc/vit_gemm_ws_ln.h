// vit_gemm_ws_ln.h -- the attention projection of ViT-S with LayerNorm-2 in its epilogue: a weight-stationary GEMM whose workgroup
// owns WHOLE rows (N = K = 384).
#pragma once
#include <utility>
#include "vit_gemm_ws.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// C[M][384] = A[M][384] . Wt[384][384]^T, EPI_DELTA arithmetic, then x += delta and LayerNorm of the updated row -- one launch
// where gemm_ws_kernel<T, EPI_DELTA> + layernorm_kernel were two: the 16-bit `delta` never reaches memory (1.12 GB of the 4.48 GB
// the pair moves per block and 90 frames), and each token tile is fetched once instead of once per column group.
//
// gemm_ws_kernel splits N = 384 over two column groups, so no workgroup there sees a whole row.  Here one workgroup of four waves
// owns all 384 features: wave w keeps features 96 w .. 96 w + 95 in registers for its whole chunk of token tiles -- three 32-row
// weight tiles x 24 k-steps x 4 = 288 registers, 240 of them AGPRs (loaded there by asm, as in gemm_ws_kernel), the rest wherever
// the compiler puts them.  Token tiles, their LDS image, the fragment reads and the order of the 24 k-steps of every accumulator
// are gemm_ws_kernel's, the update is its T((acc + bias) * gamma): the 16-bit delta is bit-identical to the two-launch form's.
//
// A step (one tile of 32 tokens, one barrier):
//   1. the eight rows of x this wave will normalise are requested (64 VGPRs per lane, 48 KB per CU) -- they land under the MFMAs
//   2. the tile after next is requested by descriptor LDS-DMA (two tiles in flight, 48 KB per CU)
//   3. 72 MFMAs 32x32x16, one ds_read_b128 per k-step feeding three of them
//   4. the update goes as 16-bit values into an LDS staging tile [32][384] (padded pitch, double-buffered)
//   5. vmcnt + barrier: the next token tile has landed, the staged tile is complete
//   6. wave w takes rows 8 w .. 8 w + 7 of the staged tile: x += float(delta), x written back, saturation test, statistics and the
//      normalised 16-bit row by layernorm_kernel's own expressions and lane -> column map (lane c: columns 4 c .. 4 c + 3, lanes
//      0-31 also 256 + 4 c ..) -- the text of gemm_wide_delta_kernel's FUSE_LN pass, copied (sharing it as a helper would change
//      the schedule of that instantiation, see the notes there): bit-identical rows.
// The launch moves 3.36 GB per block and 90 frames, 144 KB per CU and step: ~7 us at the HBM rate against ~2 us of matrix and
// vector work, so the schedule inside a step is the compiler's.
// ---------------------------------------------------------------------------------------------------------------
constexpr int WL_N = WS_K;                          // output features = K = 384
constexpr int WL_WCOLS = WL_N / 4;                  // features per wave
constexpr int WL_RT = WL_WCOLS / 32;                // 32-row weight tiles per wave
constexpr int WL_AGPR_FRAGS = 60;                   // weight fragments (of WL_RT x WS_KS = 72) pinned to AGPRs: 240 of the 256
constexpr int WL_PITCH = WL_N * 2 + 16;             // staged row: 768 B of payload + 16 (16-byte writes of 32 tokens spread over the banks)
constexpr int WL_STAGE_BYTES = WS_ROWS * WL_PITCH;
constexpr int WL_MAX_TPC = 65536;                   // token tiles per chunk: 32-bit byte offsets inside a chunk (65536 x 24 KB)
static_assert(WL_RT * 32 * 4 == WL_N, "four waves of whole 32-row weight tiles");

template <typename T>
__global__ __launch_bounds__(256) void gemm_ws_ln_kernel(const T* __restrict__ A, const T* __restrict__ Wt, long long M, GemmEpi<T> e,
                                                         int tiles_per_chunk) {
    typedef typename Vec<T>::t8 T8;
    typedef typename Vec<T>::t4 T4;
    (void)sizeof(T8); (void)sizeof(T4);
    operand_mode<T>();
    __shared__ __attribute__((aligned(1024))) unsigned char toks[3][WS_TILE_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char stage[2][WL_STAGE_BYTES];
    __shared__ __attribute__((aligned(16))) float s_bias[WL_N], s_gamma[WL_N];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int n0 = w * WL_WCOLS;
    const long long total_tiles = (M + WS_ROWS - 1) / WS_ROWS;
    const long long tile0 = (long long)blockIdx.x * tiles_per_chunk;
    if (tile0 >= total_tiles) return;
    const int NT = (int)((total_tiles - tile0) < tiles_per_chunk ? (total_tiles - tile0) : tiles_per_chunk);
    // weights: MFMA row i of row tile t carries output feature n0 + 32 t + nl(i) (gemm_ws_kernel's permutation: in D a lane (token j,
    // half h) holds the 16 CONSECUTIVE features n0 + 32 t + 16 h + r)
    const int nl = (j & 3) + 4 * (j >> 3) + 16 * ((j >> 2) & 1);
    T8 wf[WL_RT][WS_KS];
#pragma unroll
    for (int t = 0; t < WL_RT; ++t) {
        const T* wp = Wt + (size_t)(n0 + t * 32 + nl) * WS_K + h * 8;
#pragma unroll
        for (int ks = 0; ks < WS_KS; ++ks) {
            if (t * WS_KS + ks < WL_AGPR_FRAGS) asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(wf[t][ks]) : "v"(wp + ks * 16) : "memory");
            else wf[t][ks] = *reinterpret_cast<const T8*>(wp + ks * 16);
        }
    }
    // (the asm loads are invisible to the compiler's vmcnt bookkeeping: wait, then re-define every loaded register behind the wait --
    //  gemm_ws_kernel)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int t = 0; t < WL_RT; ++t)
#pragma unroll
        for (int ks = 0; ks < WS_KS; ++ks)
            if (t * WS_KS + ks < WL_AGPR_FRAGS) asm volatile("" : "+a"(wf[t][ks]));
    for (int i = tid; i < WL_N; i += 256) {
        s_bias[i] = e.bias ? e.bias[i] : 0.f;
        s_gamma[i] = e.gamma[i];
    }
    // LayerNorm parameters of this lane's columns.  (Used by an empty asm at once: the compiler's wait for these loads then stands
    // here and not at their first use inside the loop, where it would drain the requests in flight at every step.)
    const f4 ga = *reinterpret_cast<const f4*>(e.ln_w + lane * 4), ba = *reinterpret_cast<const f4*>(e.ln_b + lane * 4);
    const f4 gb = *reinterpret_cast<const f4*>(e.ln_w + 256 + (lane & 31) * 4), bb = *reinterpret_cast<const f4*>(e.ln_b + 256 + (lane & 31) * 4);
    asm volatile("" ::"v"(ga), "v"(ba), "v"(gb), "v"(bb));
    // token tiles: gemm_ws_kernel's requests and LDS image (region (g, c) of 1 KB holds tokens 4g .. 4g+3, pieces 16c .. 16c+15; piece pp
    // of token tt at slot ((pp + g) & 15) * 4 + tt); wave w requests regions 2 w and 2 w + 1.  Rows of the LAST tile past M - 1 read row M - 1.
    const unsigned lds_base = (unsigned)(size_t)&toks[0][0];
    const int l_tt = lane & 3, l_pp = lane >> 2;
    const dtk_u4 srd = dtk_make_srd(A + tile0 * WS_ROWS * WS_K);
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
    };
    // B-operand fragment of k-step ks for lane (token j, half h): piece 2 ks + h -> region column c = ks >> 3
    unsigned frag_off[8];
#pragma unroll
    for (int k8 = 0; k8 < 8; ++k8)
        frag_off[k8] = (unsigned)((j >> 2) * 3 * 1024 + ((((2 * k8 + h + (j >> 2)) & 15) * 4 + (j & 3)) * 16));
    bool sat = false;
    // three token buffers, tiles requested two steps ahead.  The wait before a step's barrier must prove that the NEXT tile has landed:
    // loads retire in order among themselves, and the only loads issued behind that tile's requests are this step's rows of x and
    // then the six requests of the tile after next (stores only add to the count) -- so vmcnt(WS_LQ) is sufficient, and it covers x.
    // None of these loads is the compiler's: the loop must hold no s_waitcnt vmcnt but the one of step 5.
    issue(0, 0);
    issue(min(1, NT - 1), 1);
    dtk_vm_wait<WS_LQ>();
    __syncthreads();   // (also publishes s_bias / s_gamma)
    int b0 = 0;
    for (int n = 0; n < NT; ++n) {
        const int b2 = b0 == 0 ? 2 : b0 - 1;   // (b0 + 2) % 3: the buffer of the tile consumed in the previous step
        // ---- 1. this wave's eight rows of x (tail rows read row M - 1 and store nothing; lanes 32-63 repeat the second piece of lanes
        //         0-31 and never use it).  By asm, like the weights: loads the compiler counts would make it wait for them row by row
        //         in step 6 with vmcnt values that know nothing of the tile requests and so drain them, and the stores of the rows
        //         before, at every row.  The vmcnt of step 5 covers them; they are re-defined behind it.
        const long long rb = (tile0 + n) * WS_ROWS + 8 * w;
        f4 xa[8], xb[8];
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            const float* xp = e.ln_x + min(rb + rr, M - 1) * WL_N;
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(xa[rr]) : "v"(xp + lane * 4) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(xb[rr]) : "v"(xp + 256 + (lane & 31) * 4) : "memory");
        }
        // ---- 2. the tile after next (past the chunk's end: a harmless repeat keeps the request count per step uniform)
        issue(min(n + 2, NT - 1), b2);
        // ---- 3. the MFMAs of tile n: every accumulator sums its k-steps in ascending order from a zero C operand (gemm_ws_kernel)
        f16v acc[WL_RT];
        {
            const unsigned char* base = &toks[0][0] + b0 * WS_TILE_BYTES;
            const f16v zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // inline constant C
            T8 b[3];
            b[0] = *reinterpret_cast<const T8*>(base + frag_off[0]);
            b[1] = *reinterpret_cast<const T8*>(base + frag_off[1]);
#pragma unroll
            for (int ks = 0; ks < WS_KS; ++ks) {
                if (ks + 2 < WS_KS)
                    b[(ks + 2) % 3] = *reinterpret_cast<const T8*>(base + frag_off[(ks + 2) & 7] + ((ks + 2) >> 3) * 1024);
#pragma unroll
                for (int t = 0; t < WL_RT; ++t) acc[t] = mfma32(wf[t][ks], b[ks % 3], ks == 0 ? zero16 : acc[t]);
            }
        }
        // ---- 4. the update as 16-bit values into the staging tile: token j, features n0 + 32 t + 16 h .. + 15
        {
            unsigned char* const sw = &stage[n & 1][0] + j * WL_PITCH + (n0 + 16 * h) * 2;
#pragma unroll
            for (int t = 0; t < WL_RT; ++t)
#pragma unroll
                for (int hv = 0; hv < 2; ++hv) {
                    const int fb = n0 + 32 * t + 16 * h + 8 * hv;
                    const float4 b0v = *reinterpret_cast<const float4*>(&s_bias[fb]), b1v = *reinterpret_cast<const float4*>(&s_bias[fb + 4]);
                    const float4 g0v = *reinterpret_cast<const float4*>(&s_gamma[fb]), g1v = *reinterpret_cast<const float4*>(&s_gamma[fb + 4]);
                    const float bi[8] = {b0v.x, b0v.y, b0v.z, b0v.w, b1v.x, b1v.y, b1v.z, b1v.w};
                    const float gm[8] = {g0v.x, g0v.y, g0v.z, g0v.w, g1v.x, g1v.y, g1v.z, g1v.w};
                    T8 o;
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const float v0 = acc[t][8 * hv + r] + bi[r];
                        o[r] = (T)(v0 * gm[r]);
                    }
                    *reinterpret_cast<T8*>(sw + 64 * t + 16 * hv) = o;
                }
        }
        // ---- 5. tile n + 1 and this step's rows of x have landed; the staged tile is complete
        dtk_vm_wait<WS_LQ>();
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) asm volatile("" : "+v"(xa[rr]), "+v"(xb[rr]));
        __syncthreads();
        // ---- 6. LayerNorm of rows 8 w .. 8 w + 7 of the staged tile (gemm_wide_delta_kernel's FUSE_LN text)
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            const long long row = rb + rr;
            if (row >= M) continue;   // wave-uniform (the last tile's tail)
            const unsigned char* sp = &stage[n & 1][0] + (8 * w + rr) * WL_PITCH + lane * 8;
            f4 v[2] = {xa[rr], xb[rr]};
            float s = 0.f;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                if (it == 0 || lane < 32) {
                    const T4 d = *reinterpret_cast<const T4*>(sp + it * 512);
                    const float d0 = (float)d[0], d1 = (float)d[1], d2 = (float)d[2], d3 = (float)d[3];
                    sat |= update_saturated<T>(d0, d1, d2, d3);
                    v[it].x += d0; v[it].y += d1; v[it].z += d2; v[it].w += d3;
                    *reinterpret_cast<f4*>(e.ln_x + row * WL_N + it * 256 + lane * 4) = v[it];
                    s += (v[it].x + v[it].y) + (v[it].z + v[it].w);
                }
            }
            const float mean = wave_sum(s) / (float)WL_N;
            float q = 0.f;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                if (it == 0 || lane < 32) {
                    const float a = v[it].x - mean, b = v[it].y - mean, cc = v[it].z - mean, d = v[it].w - mean;
                    q += (a * a + b * b) + (cc * cc + d * d);
                }
            }
            const float rstd = rsqrtf(wave_sum(q) / (float)WL_N + e.ln_eps);
            T* o = e.ln_out + row * WL_N;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                if (it == 0 || lane < 32) {
                    const f4 g = it ? gb : ga, b = it ? bb : ba;
                    T4 r = {(T)((v[it].x - mean) * rstd * g.x + b.x), (T)((v[it].y - mean) * rstd * g.y + b.y),
                             (T)((v[it].z - mean) * rstd * g.z + b.z), (T)((v[it].w - mean) * rstd * g.w + b.w)};
                    *reinterpret_cast<T4*>(o + it * 256 + lane * 4) = r;
                }
            }
        }
        b0 = b0 == 2 ? 0 : b0 + 1;
    }
    if (IsF16<T>::value && e.ln_ovf && __any(sat) && lane == 0) atomicOr(e.ln_ovf, 1);
    dtk_vm_wait<0>();   // (the repeated requests of the last two steps still write LDS)
}

// grid and token tiles per chunk: consecutive tiles per workgroup, one workgroup per CU of the device (one resident round)
inline std::pair<dim3, int> gemm_ws_ln_grid(long long rows) {
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        return n;
    }();
    const long long tiles = dtk_cdiv(rows, WS_ROWS);
    int tpc = (int)dtk_cdiv(tiles, cus);
    if (tpc > WL_MAX_TPC) tpc = WL_MAX_TPC;
    return std::make_pair(dim3((unsigned)dtk_cdiv(tiles, tpc)), tpc);
}

}  // namespace
