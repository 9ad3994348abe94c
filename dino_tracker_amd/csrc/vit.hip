// vit.hip -- P1: DINOv2 ViT encoder as driven by VitExtractor (models/extractor.py:41-150, utils.py:33-72):
// overlapping patch embedding (14x14, stride 7) of ImageNet-normalised frames + interpolated position encoding,
// `depth` transformer blocks (LN -> QKV -> MHSA -> proj -> LayerScale -> +res; LN -> fc1 -> GELU -> fc2 -> LayerScale
// -> +res; ViT-g/14: LN -> w12 -> silu(gate) * value -> w3 instead, dtk_vit_model.ffn), output = residual stream after the last requested block (no final norm), CLS included
// (and, DINOv2 with registers, the dtk_vit_model.n_registers register rows between CLS and the patches: S = 1 + R + ph * pw).
//
// This file is the host side: the workspace plan, the kernel choice of a pass (GemmPath, launch_gemm / launch_gemm_split), the one
// description of every GEMM role (run_gemm / run_gemm_split: vit_run and the stage API dtk_vit_gemm both go through it), vit_run, the ABI.
//   vit_patch_embed.h   exact fp32 implicit GEMM on the f32-input MFMA (K = 3*14*14 = 588), mean/std fused in the load, or on the split-fp16 MFMA
//   vit_rowwise.h       layernorm_kernel: one wave per token, fp32 statistics, 16-bit output; the row in NIT float4 per lane (D <= 1024: 4,
//                       D <= 1536: 6); the final residual update, tap, prefix (CLS + registers) drop, range scan, zero fill
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
#include "vit_rowwise.h"
#include "vit_patch_embed.h"
#include "vit_gemm_tiled.h"
#include "vit_gemm_ws.h"
#include "vit_gemm_ws_ln.h"
#include "vit_gemm_wide.h"
#include "vit_split.h"

namespace {

// Frames per pass of the encoder: large batches give the weight-stationary GEMMs long token chunks per workgroup (their weights
// are loaded once per chunk).  Round 4: 90 (a whole benchmark video: 7.8 GB of activations, 2.7 % of the 288 GB) instead of
// 30 -- fewer, longer launches: the attention's last partial round of workgroups weighs 0.7 % instead of 2.2 %, the
// weight-stationary GEMMs load their weights a third as often; 301.4 -> 294.8 ms per step (profiles/r04_frame_batch_sweep.txt).
constexpr int VIT_FRAME_BATCH = 90;
constexpr int VIT_MAX_REGISTERS = 16;   // dtk_vit_model.n_registers (the hub's register models have 4)

struct VitPlan {
    int S, Sp, FB;
    size_t x, xn, q, k, vt, ao, hid, delta, total;
    bool split;                                    // some block runs on split operands (dtk_vit_layer.qkv_w_lo): the lo planes exist
    size_t xn_lo, q_lo, k_lo, vt_lo, ao_lo, hid_lo;
};

inline bool vit_layer_split(const dtk_vit_layer& L) { return L.qkv_w_lo != nullptr; }

VitPlan vit_plan(const dtk_vit_model* m, int ph, int pw, int frames) {
    VitPlan p;
    p.S = 1 + m->n_registers + ph * pw;   // CLS, the registers (DINOv2 with registers; 0 for the plain models), the patches
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
// the same stage of a split block (vit_run, dtk_vit_attention_split): hi / lo planes of every operand and of the output
template <typename T>
int attention_split_launch(const T* q, const T* q_lo, const T* k, const T* k_lo, const T* vt, const T* vt_lo, T* o, T* o_lo, int frames,
                           int heads, int S, int Sp, hipStream_t st) {
    const int nqb = dtk_cdiv(Sp, 128);
    DTK_LAUNCH("vit_attention_split", attention_split_kernel<T>, dim3((unsigned)(frames * heads * nqb)), dim3(256), 0, st, q, q_lo, k, k_lo,
               vt, vt_lo, o, o_lo, S, Sp, heads, nqb);
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
//   gemm_ws96_runs (fc1, qkv; not ws_v1)             gemm_ws_kernel<T, EPI, 3, true, 3>                  gemm_ws96_plan(N)   x 256
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
// (gemm_ws_kernel's QKV epilogue steps (frame, position) a tile at a time and lets a tile cross ONE frame end: S >= WS_ROWS.
//  SEVERAL shorter frames -- under 49 x 49 pixels -- put Q / K rows into the padding of the wrong frame; the tiled kernel divides per row.)
inline bool gemm_ws_fits(int epi, long long rows, int S) { return epi != EPI_QKV || S >= WS_ROWS || rows <= S; }
// Does this GEMM run the 96-features-per-wave form (RT = 3) of gemm_ws_kernel?  The one predicate of launch_gemm and of
// dtk_vit_gemm_ws_plan: fc1 and qkv of the weight-stationary width, N a multiple of 384, no A / B switch.
inline bool gemm_ws96_runs(const GemmPath& path, int epi, long long rows, int N, int K, int S, int no_store) {
    return gemm_ws96_role(epi) && path.ws && K == WS_K && gemm_ws_fits(epi, rows, S) && !path.ws_v1 && gemm_ws96_fits(N) && !DTK_DBG(no_store, 128);
}

template <typename T, int EPI>
int launch_gemm(const char* name, const GemmPath& path, const T* A, const T* W, long long rows, int N, int K, const GemmEpi<T>& e,
                hipStream_t st) {
    if constexpr (EPI != EPI_F32) {
        const bool ws_fits = gemm_ws_fits(EPI, rows, e.S);
        if constexpr (EPI == EPI_DELTA) {
            if (path.ws && K == WS_K && N == WS_K && e.ln_out) {
                const auto gr = gemm_ws_ln_grid(rows);
                DTK_LAUNCH(name, (gemm_ws_ln_kernel<T>), gr.first, dim3(256), 0, st, A, W, rows, e, gr.second);
                return DTK_OK;
            }
        }
        if constexpr (gemm_ws96_role(EPI)) {   // 96 features per wave, chunks by plan; every A / B switch keeps the 64-feature form
            if (gemm_ws96_runs(path, EPI, rows, N, K, e.S, e.no_store)) {
                const Ws96Plan plan = gemm_ws96_plan(N, rows);
                DTK_LAUNCH(name, (gemm_ws_kernel<T, EPI, 3, true, 3>), gemm_ws96_grid(plan), dim3(256), 0, st, A, W, rows, N, e, plan);
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

// ---- one GEMM of a block, by role ---------------------------------------------------------------------------------------------------
// What a role's GEMM is -- shape, epilogue descriptor, launch name -- is written ONCE, in run_gemm (fast blocks) and run_gemm_split
// (split blocks), for the encoder pass (vit_run) and the stage API (dtk_vit_gemm / dtk_vit_gemm_split) alike.  Both hand over a
// dtk_vit_gemm_args (include/dtk.h); its flags and operand_type arrive here as `path` and T, and where the fused LayerNorm may run
// is the caller's decision: it sets ln_out or not.
constexpr int VITG_HIDDEN = 4096;   // upstream vit_giant2: (int(4 * 1536 * 2 / 3) + 7) / 8 * 8
constexpr int VIT_D_HEAD = 64;
constexpr float VIT_QSCALE = 0.125f * 1.4426950408889634f;   // log2(e) / sqrt(d_head) on Q: the attention's softmax runs in the exp2 domain
struct GemmShape { int N, K; };   // C[rows][N] = A[rows][K] . W[N][K]^T of a role in a model of width D whose feed-forward is `hidden` wide
inline GemmShape gemm_shape(int role, int D, int hidden) {
    switch (role) {
        case DTK_VIT_GEMM_QKV:
        case DTK_VIT_GEMM_QKV_FACET: return {3 * D, D};
        case DTK_VIT_GEMM_PROJ: return {D, D};
        case DTK_VIT_GEMM_FC1: return {hidden, D};
        case DTK_VIT_GEMM_FC1_SWIGLU: return {2 * hidden, D};   // the PACKED w12
        default: return {D, hidden};                            // FC2, FC2_SWIGLU
    }
}

// no_store: the DTK_DEV store / main-loop ablations (GemmEpi::no_store), vit_run only
template <typename T>
int run_gemm(const dtk_vit_gemm_args& g, const GemmPath& path, int hidden, hipStream_t st, int no_store = 0) {
    const GemmShape sh = gemm_shape(g.role, g.D, hidden);
    const T *A = reinterpret_cast<const T*>(g.a), *W = reinterpret_cast<const T*>(g.w);
    int* const epi_ovf = IsF16<T>::value ? g.ovf : nullptr;
    GemmEpi<T> e{};
    e.bias = g.bias; e.no_store = no_store;
    switch (g.role) {
        case DTK_VIT_GEMM_QKV:
            e.q = reinterpret_cast<T*>(g.q); e.k = reinterpret_cast<T*>(g.k); e.vt = reinterpret_cast<T*>(g.vt);
            e.S = g.S; e.Sp = g.Sp; e.heads = g.D / VIT_D_HEAD; e.D = g.D; e.qscale = VIT_QSCALE; e.ovf = epi_ovf;
            return launch_gemm<T, EPI_QKV>("vit_gemm_qkv", path, A, W, g.rows, sh.N, sh.K, e, st);
        case DTK_VIT_GEMM_QKV_FACET:   // the qkv hook of the reference (models/extractor.py:107-118), fp32 out
            e.out_f32 = g.out_f32;
            return launch_gemm<T, EPI_F32>("vit_gemm_qkv_facet", path, A, W, g.rows, sh.N, sh.K, e, st);
        case DTK_VIT_GEMM_FC1:
        case DTK_VIT_GEMM_FC1_SWIGLU:
            e.out = reinterpret_cast<T*>(g.out); e.ovf = epi_ovf;
            return g.role == DTK_VIT_GEMM_FC1 ? launch_gemm<T, EPI_GELU>("vit_gemm_fc1", path, A, W, g.rows, sh.N, sh.K, e, st)
                                              : launch_gemm_swiglu<T>("vit_gemm_fc1", path, A, W, g.rows, sh.N, sh.K, e, st);
        default:   // PROJ, FC2, FC2_SWIGLU: the LayerScale'd residual update
            e.delta = reinterpret_cast<T*>(g.out); e.gamma = g.gamma;
            if (g.ln_out) {   // the LayerNorm inside the epilogue: x += update (not stored), ln_out = the normalised rows
                e.ln_x = g.ln_x; e.ln_w = g.ln_w; e.ln_b = g.ln_b; e.ln_out = reinterpret_cast<T*>(g.ln_out); e.ln_eps = g.ln_eps;
                e.ln_ovf = g.ovf;
            }
            return launch_gemm<T, EPI_DELTA>(g.role == DTK_VIT_GEMM_PROJ ? "vit_gemm_proj" : "vit_gemm_fc2", path, A, W, g.rows, sh.N, sh.K, e, st);
    }
}

// The same roles on hi / lo planes (vit_split.h); the residual roles add their update to the fp32 stream g.x.
template <typename T>
int run_gemm_split(const dtk_vit_gemm_args& g, const GemmPath& path, int hidden, hipStream_t st) {
    const GemmShape sh = gemm_shape(g.role, g.D, hidden);
    const T *Ah = reinterpret_cast<const T*>(g.a), *Al = reinterpret_cast<const T*>(g.a_lo);
    const T *Wh = reinterpret_cast<const T*>(g.w), *Wl = reinterpret_cast<const T*>(g.w_lo);
    int* const epi_ovf = IsF16<T>::value ? g.ovf : nullptr;
    SplitEpi<T> se{};
    se.bias = g.bias; se.inv_wscale = 1.f / (g.w_scale > 0.f ? g.w_scale : 1.f);
    switch (g.role) {
        case DTK_VIT_GEMM_QKV:
            se.q_hi = reinterpret_cast<T*>(g.q); se.q_lo = reinterpret_cast<T*>(g.q_lo); se.k_hi = reinterpret_cast<T*>(g.k);
            se.k_lo = reinterpret_cast<T*>(g.k_lo); se.vt_hi = reinterpret_cast<T*>(g.vt); se.vt_lo = reinterpret_cast<T*>(g.vt_lo);
            se.S = g.S; se.Sp = g.Sp; se.heads = g.D / VIT_D_HEAD; se.D = g.D; se.qscale = VIT_QSCALE; se.ovf = epi_ovf;
            return launch_gemm_split<T, SEPI_QKV>("vit_gemm_qkv_split", path, Ah, Al, Wh, Wl, g.rows, sh.N, sh.K, se, st);
        case DTK_VIT_GEMM_QKV_FACET:
            se.out_f32 = g.out_f32;
            return launch_gemm_split<T, SEPI_F32>("vit_gemm_qkv_facet", path, Ah, Al, Wh, Wl, g.rows, sh.N, sh.K, se, st);
        case DTK_VIT_GEMM_FC1:
        case DTK_VIT_GEMM_FC1_SWIGLU:
            se.out_hi = reinterpret_cast<T*>(g.out); se.out_lo = reinterpret_cast<T*>(g.out_lo); se.ovf = epi_ovf;
            return g.role == DTK_VIT_GEMM_FC1
                       ? launch_gemm_split<T, SEPI_GELU>("vit_gemm_fc1_split", path, Ah, Al, Wh, Wl, g.rows, sh.N, sh.K, se, st)
                       : launch_gemm_split<T, SEPI_SWIGLU>("vit_gemm_fc1_split", path, Ah, Al, Wh, Wl, g.rows, sh.N, sh.K, se, st);
        default:
            se.x = g.x; se.gamma = g.gamma;
            return launch_gemm_split<T, SEPI_RESID>(g.role == DTK_VIT_GEMM_PROJ ? "vit_gemm_proj_split" : "vit_gemm_fc2_split", path, Ah, Al,
                                                    Wh, Wl, g.rows, sh.N, sh.K, se, st);
    }
}

template <typename T>
int vit_run(const dtk_vit_model* m, const float* frames, int nframes, int video_h, int video_w, float* tokens_out,
            float* feat_out, float* qkv_out, unsigned char* ws, const VitPlan& p, int ph, int pw, hipStream_t st) {
    const int HW = ph * pw, D = m->D;
    // the feed-forward: GELU MLP (hidden 4 D) or, ViT-g, SwiGLU -- fc1_w is then the PACKED w12 [2 hidden][D] (include/dtk.h) and the
    // GEMM's epilogue writes silu(gate) * value, fc2_w is w3 [D][hidden]; `hid` is sized for 4 D >= hidden
    const bool swiglu = m->ffn == DTK_VIT_FFN_SWIGLU;
    const int HID = m->hidden > 0 ? m->hidden : 4 * D;
    const int FC1 = swiglu ? DTK_VIT_GEMM_FC1_SWIGLU : DTK_VIT_GEMM_FC1, FC2 = swiglu ? DTK_VIT_GEMM_FC2_SWIGLU : DTK_VIT_GEMM_FC2;
    float* x = reinterpret_cast<float*>(ws + p.x);
    auto at = [&](size_t off) { return reinterpret_cast<T*>(ws + off); };
    T *xn = at(p.xn), *q = at(p.q), *k = at(p.k), *vt = at(p.vt), *ao = at(p.ao), *hid = at(p.hid), *delta = at(p.delta);
    T *xn_lo = at(p.xn_lo), *q_lo = at(p.q_lo), *k_lo = at(p.k_lo), *vt_lo = at(p.vt_lo), *ao_lo = at(p.ao_lo), *hid_lo = at(p.hid_lo);
    T* const none = nullptr;
    int* ovf = m->overflow;
    // Saturation of Q / K / V^T and of the MLP hidden (overflow bits 2 / 4): tracked for EVERY value of EVERY frame inside the
    // epilogues of the QKV and fc1 GEMMs (GemmEpi::ovf, round 5: four v_max3 per eight values, no extra pass; rounds 3-4 scanned
    // the first frame of a call only, so a later frame could saturate silently).  DTK_VIT_CHECK_RANGE additionally scans the
    // stored tensors of every block (a pass over 1.3 GB per block and 30 frames): the cross-check of the tests.
    const bool scan_all = ovf && (m->flags & DTK_VIT_CHECK_RANGE);
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
        // (`hid` and `delta` are unused until the first block: the scratch of the split-fp16 patch embedding)
        if (launch_patch_embed(m, frames + (size_t)f0 * 3 * video_h * video_w, nf, video_h, video_w, ph, pw, x, hid, p.delta - p.hid, delta,
                               p.total - p.delta, st)) return DTK_E_HIP;
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
            const bool facet = qkv_out && l == m->depth - 1;   // the qkv hook: the last block's, fp32
            // what every GEMM of this block is given (a role reads its own operands only), and one GEMM's: role, A, W, bias (and lo planes)
            dtk_vit_gemm_args block{};
            block.D = D; block.rows = rows; block.S = S; block.Sp = Sp; block.ln_eps = m->ln_eps; block.w_scale = L.w_scale; block.ovf = ovf;
            block.q = q; block.k = k; block.vt = vt; block.q_lo = q_lo; block.k_lo = k_lo; block.vt_lo = vt_lo; block.x = x;
            block.out_f32 = facet ? qkv_out + (size_t)f0 * S * 3 * D : nullptr;
            auto gemm_of = [&](int role, const T* a, const T* a_lo, const void* w, const void* w_lo, const float* bias, const float* gamma = nullptr) {
                dtk_vit_gemm_args g = block;
                g.role = role; g.a = a; g.a_lo = a_lo; g.w = w; g.w_lo = w_lo; g.bias = bias; g.gamma = gamma;
                return g;
            };
            dtk_vit_gemm_args g;
            if (vit_layer_split(L)) {
                // ---- the escalated precision (vit_split.h): every product on hi + lo operands, updates straight into x ----
                if (launch_layernorm<T>(x, pending ? delta : none, L.ln1_w, L.ln1_b, xn, xn_lo, rows, D, m->ln_eps, ovf, st)) return DTK_E_HIP;
                pending = false;
                if (facet && run_gemm_split<T>(gemm_of(DTK_VIT_GEMM_QKV_FACET, xn, xn_lo, L.qkv_w, L.qkv_w_lo, L.qkv_b), path, HID, st))
                    return DTK_E_HIP;
                if (run_gemm_split<T>(gemm_of(DTK_VIT_GEMM_QKV, xn, xn_lo, L.qkv_w, L.qkv_w_lo, L.qkv_b), path, HID, st)) return DTK_E_HIP;
                if (attention_split_launch<T>(q, q_lo, k, k_lo, vt, vt_lo, ao, ao_lo, nf, m->heads, S, Sp, st)) return DTK_E_HIP;
                if (run_gemm_split<T>(gemm_of(DTK_VIT_GEMM_PROJ, ao, ao_lo, L.proj_w, L.proj_w_lo, L.proj_b, L.ls1), path, HID, st)) return DTK_E_HIP;
                if (launch_layernorm<T>(x, none, L.ln2_w, L.ln2_b, xn, xn_lo, rows, D, m->ln_eps, ovf, st)) return DTK_E_HIP;
                g = gemm_of(FC1, xn, xn_lo, L.fc1_w, L.fc1_w_lo, L.fc1_b);
                g.out = hid; g.out_lo = hid_lo;
                if (run_gemm_split<T>(g, path, HID, st)) return DTK_E_HIP;
                if (run_gemm_split<T>(gemm_of(FC2, hid, hid_lo, L.fc2_w, L.fc2_w_lo, L.fc2_b, L.ls2), path, HID, st)) return DTK_E_HIP;
                if (tap(l, false)) return DTK_E_HIP;
                continue;
            }
            if (!ln1_done && launch_layernorm<T>(x, pending ? delta : none, L.ln1_w, L.ln1_b, xn, none, rows, D, m->ln_eps, ovf, st))
                return DTK_E_HIP;
            ln1_done = false;
            pending = true;
            if (facet && run_gemm<T>(gemm_of(DTK_VIT_GEMM_QKV_FACET, xn, none, L.qkv_w, nullptr, L.qkv_b), path, HID, st)) return DTK_E_HIP;
            if (run_gemm<T>(gemm_of(DTK_VIT_GEMM_QKV, xn, none, L.qkv_w, nullptr, L.qkv_b), path, HID, st, dbg_ns)) return DTK_E_HIP;
            if (scan_all && scan_range(q, (long long)(p.ao - p.q) / 2, 2)) return DTK_E_HIP;
            if (attention_launch(q, k, vt, ao, S, Sp, m->heads, D, nf * m->heads, (m->flags & DTK_VIT_ATTENTION_V4) != 0, st)) return DTK_E_HIP;
            g = gemm_of(DTK_VIT_GEMM_PROJ, ao, none, L.proj_w, nullptr, L.proj_b, L.ls1);
            g.out = delta;
            // LayerNorm-2 runs inside the projection's epilogue (gemm_ws_ln_kernel: x += update, xn = the normalised rows; the update is
            // not stored) -- `pending` / `ln1_done` speak of fc2's update and LayerNorm-1 only, and stay as they are
            if (path.proj_ln) { g.ln_x = x; g.ln_w = L.ln2_w; g.ln_b = L.ln2_b; g.ln_out = xn; }
            if (run_gemm<T>(g, path, HID, st, dbg_ns)) return DTK_E_HIP;
            if (!path.proj_ln && launch_layernorm<T>(x, delta, L.ln2_w, L.ln2_b, xn, none, rows, D, m->ln_eps, ovf, st)) return DTK_E_HIP;
            g = gemm_of(FC1, xn, none, L.fc1_w, nullptr, L.fc1_b);
            g.out = hid;
            if (run_gemm<T>(g, path, HID, st, dbg_ns)) return DTK_E_HIP;
            if (scan_all && scan_range(hid, rows * HID, 4)) return DTK_E_HIP;
            g = gemm_of(FC2, hid, none, L.fc2_w, nullptr, L.fc2_b, L.ls2);
            g.out = delta;
            // round 6: the LayerNorm of the next block runs inside fc2's epilogue when that block is a fast one (the split blocks
            // have their own LayerNorm: hi / lo planes); the last block's update goes to the outputs (below)
            if (path.fc2_ln && l + 1 < m->depth && !vit_layer_split(m->layers[l + 1])) {
                const dtk_vit_layer& Ln = m->layers[l + 1];
                g.ln_x = x; g.ln_w = Ln.ln1_w; g.ln_b = Ln.ln1_b; g.ln_out = xn;
                pending = false;      // x is up to date ...
                ln1_done = true;      // ... and xn holds the next block's normalised rows
            }
            if (run_gemm<T>(g, path, HID, st, dbg_ns)) return DTK_E_HIP;
            if (tap(l, pending)) return DTK_E_HIP;
        }
        if (pending && (tokens_out || feat_out)) {
            // the last MLP's residual update, written straight to the outputs (x itself is dead after the last block)
            const long long t4 = rows * (D / 4);
            DTK_LAUNCH("vit_final_update", final_update_kernel<T>, dim3(dtk_cdiv(t4, 256)), dim3(256), 0, st, x, (const T*)delta,
                       tokens_out ? tokens_out + (size_t)f0 * S * D : (float*)nullptr,
                       feat_out ? feat_out + (size_t)f0 * HW * D : (float*)nullptr, S, D, t4, ovf, S - HW);
        } else {   // depth 0 (embedding + position encoding only) or a split last block: no pending update
            if (pending &&   // (qkv_out only: keep the residual-update check of the last block)
                launch_layernorm<T>(x, delta, (const float*)nullptr, (const float*)nullptr, none, none, rows, D, m->ln_eps, ovf, st))
                return DTK_E_HIP;
            if (tokens_out)
                DTK_HIP(hipMemcpyAsync(tokens_out + (size_t)f0 * S * D, x, (size_t)rows * D * sizeof(float),
                                       hipMemcpyDeviceToDevice, st));
            if (feat_out) {
                const long long total4 = (long long)nf * HW * (D / 4);
                DTK_LAUNCH("vit_drop_cls", drop_cls_kernel, dim3(dtk_cdiv(total4, 256)), dim3(256), 0, st, x,
                           feat_out + (size_t)f0 * HW * D, S, D, total4, S - HW);
            }
        }
    }
    return DTK_OK;
}

// ---- one GEMM of a block on its own (dtk_vit_gemm / dtk_vit_gemm_split) ------------------------------------------------------------
// The role names the shape and the epilogue (run_gemm / run_gemm_split: vit_run's own set-up); the kernel is what launch_gemm /
// launch_gemm_split choose for a model of width D with these flags (gemm_path: the dispatch of vit_run, no second table).
int vit_gemm_check(const dtk_vit_gemm_args* g, const char* who, bool split) {
    DTK_REQUIRE(g, "%s: null pointer", who);
    DTK_REQUIRE(g->D == 384 || g->D == 768 || g->D == 1024 || g->D == 1536, "%s: D must be 384, 768 or 1024, or ViT-g's 1536 (got %d)", who, g->D);
    DTK_REQUIRE(g->operand_type == DTK_OPERAND_F16 || g->operand_type == DTK_OPERAND_BF16, "%s: operand_type", who);
    DTK_REQUIRE(g->rows > 0 && g->rows < (1ll << 31), "%s: rows", who);
    DTK_REQUIRE(g->a && g->w && (!split || (g->a_lo && g->w_lo)), "%s: null operand", who);
    const bool swiglu = g->role == DTK_VIT_GEMM_FC1_SWIGLU || g->role == DTK_VIT_GEMM_FC2_SWIGLU;
    if (swiglu) {
        DTK_REQUIRE(g->D == 1536, "%s: the SwiGLU roles are ViT-g's, D = 1536 (got %d)", who, g->D);
        if (!vit_swiglu_flags_ok(g->flags, who)) return DTK_E_INVALID;
    }
    bool update = false;   // a residual role: the only ones that may carry a fused LayerNorm
    switch (g->role) {
        case DTK_VIT_GEMM_QKV:
            DTK_REQUIRE(g->q && g->k && g->vt && (!split || (g->q_lo && g->k_lo && g->vt_lo)), "%s: QKV needs q, k and vt", who);
            DTK_REQUIRE(g->S > 0 && g->Sp >= g->S && g->Sp % 64 == 0 && g->rows % g->S == 0,
                        "%s: bad sizes (Sp %% 64 == 0, Sp >= S, rows a multiple of S)", who);
            break;
        case DTK_VIT_GEMM_QKV_FACET:
            DTK_REQUIRE(g->out_f32, "%s: QKV_FACET needs out_f32", who);
            break;
        case DTK_VIT_GEMM_FC1:
        case DTK_VIT_GEMM_FC1_SWIGLU:
            DTK_REQUIRE(g->out && (!split || g->out_lo), "%s: %s needs out", who, swiglu ? "FC1_SWIGLU" : "FC1");
            break;
        case DTK_VIT_GEMM_PROJ:
        case DTK_VIT_GEMM_FC2:
        case DTK_VIT_GEMM_FC2_SWIGLU:
            DTK_REQUIRE(g->gamma && (split ? g->x != nullptr : g->out != nullptr), "%s: %s gamma and %s", who,
                        swiglu ? "FC2_SWIGLU needs" : "PROJ / FC2 need", split ? "x" : "out");
            update = true;
            break;
        default:
            DTK_REQUIRE(false, "%s: unknown role %d", who, g->role);
    }
    if (!split && update && g->ln_out) {   // the LayerNorm inside fc2's (the next block's) or the projection's (LayerNorm-2) epilogue: where vit_run fuses it, nowhere else
        const GemmPath path = gemm_path(g->D, g->flags);
        DTK_REQUIRE(g->role == DTK_VIT_GEMM_PROJ ? path.proj_ln : path.fc2_ln,
                    "dtk_vit_gemm: the fused LayerNorm is fc2's or the projection's at D = 384 without TILED_GEMMS / GEMM_WIDE_V1 / NO_LN_FUSION (the projection's: nor GEMM_WS_V1)");
        DTK_REQUIRE(g->ln_x && g->ln_w && g->ln_b, "dtk_vit_gemm: the fused LayerNorm needs ln_x, ln_w and ln_b");
    }
    return DTK_OK;
}
inline int vit_gemm_hidden(const dtk_vit_gemm_args* g) {   // the feed-forward width the stage API's roles stand for
    return g->role == DTK_VIT_GEMM_FC1_SWIGLU || g->role == DTK_VIT_GEMM_FC2_SWIGLU ? VITG_HIDDEN : 4 * g->D;
}

// every DTK_VIT_* bit of dtk_vit_model.flags that include/dtk.h defines (bit 8 is retired and not reused)
constexpr int VIT_KNOWN_FLAGS = DTK_VIT_TILED_GEMMS | DTK_VIT_BF16 | DTK_VIT_CHECK_RANGE | DTK_VIT_GEMM_WS_V1 | DTK_VIT_ATTENTION_V4 |
                                DTK_VIT_GEMM_WIDE_V1 | DTK_VIT_NO_LN_FUSION;

// The one fork between the two operand types: f(T()) with T = __bf16 or _Float16 (a generic lambda reads T off its argument).
template <typename F> int with_operand_type(bool bf16, F&& f) { return bf16 ? f(__bf16()) : f(_Float16()); }

}  // namespace

extern "C" size_t dtk_vit_workspace_bytes(const dtk_vit_model* m, int video_h, int video_w, int frames) {
    if (!m || frames <= 0 || m->n_registers < 0 || m->n_registers > VIT_MAX_REGISTERS) return 0;
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
    DTK_REQUIRE(m->D > 0 && m->heads > 0 && m->D == m->heads * VIT_D_HEAD, "dtk_vit_forward: d_head must be 64 (D=%d heads=%d)",
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
    DTK_REQUIRE(m->n_registers >= 0 && m->n_registers <= VIT_MAX_REGISTERS, "dtk_vit_forward: n_registers = %d: 0 .. %d register tokens",
                m->n_registers, VIT_MAX_REGISTERS);
    DTK_REQUIRE(m->n_registers == 0 || m->registers, "dtk_vit_forward: n_registers = %d but registers is a null pointer", m->n_registers);
    DTK_REQUIRE(video_h >= m->patch && video_w >= m->patch, "dtk_vit_forward: frame smaller than a patch");
    const int ph = 1 + (video_h - m->patch) / m->stride, pw = 1 + (video_w - m->patch) / m->stride;
    const VitPlan p = vit_plan(m, ph, pw, nframes);
    if (workspace_bytes < p.total) {
        dtk_set_error("dtk_vit_forward: workspace %zu B < required %zu B", workspace_bytes, p.total);
        return DTK_E_WORKSPACE;
    }
    return with_operand_type((m->flags & DTK_VIT_BF16) != 0, [&](auto t) {
        return vit_run<decltype(t)>(m, frames, nframes, video_h, video_w, tokens_out, feat_out, qkv_out, reinterpret_cast<unsigned char*>(workspace),
                                    p, ph, pw, dtk_stream(stream));
    });
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
    return with_operand_type(operand_type == DTK_OPERAND_BF16, [&](auto t) {
        typedef decltype(t) T;
        return attention_launch(reinterpret_cast<const T*>(q), reinterpret_cast<const T*>(k), reinterpret_cast<const T*>(vt),
                                reinterpret_cast<T*>(out), S, Sp, heads, heads * VIT_D_HEAD, frames * heads, v4, dtk_stream(stream));
    });
}

// The same stage on split operands (vit_split.h: the escalated precision): hi / lo planes of every operand and of the output.
extern "C" int dtk_vit_attention_split(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* vt_hi,
                                       const void* vt_lo, void* out_hi, void* out_lo, int frames, int heads, int S, int Sp,
                                       int operand_type, void* stream) {
    DTK_REQUIRE(q_hi && q_lo && k_hi && k_lo && vt_hi && vt_lo && out_hi && out_lo, "dtk_vit_attention_split: null pointer");
    DTK_REQUIRE(frames > 0 && heads > 0 && S > 0 && Sp >= S && Sp % 64 == 0, "dtk_vit_attention_split: bad sizes (Sp %% 64 == 0, Sp >= S)");
    DTK_REQUIRE(operand_type == DTK_OPERAND_F16 || operand_type == DTK_OPERAND_BF16, "dtk_vit_attention_split: operand_type");
    return with_operand_type(operand_type == DTK_OPERAND_BF16, [&](auto t) {
        typedef decltype(t) T;
        return attention_split_launch<T>((const T*)q_hi, (const T*)q_lo, (const T*)k_hi, (const T*)k_lo, (const T*)vt_hi, (const T*)vt_lo,
                                         (T*)out_hi, (T*)out_lo, frames, heads, S, Sp, dtk_stream(stream));
    });
}

// One GEMM of a block on its own (tests compare every kernel form with float64 on the operands it read; layouts, set-up and dispatch
// are those of dtk_vit_forward: run_gemm).
extern "C" int dtk_vit_gemm(const dtk_vit_gemm_args* g, void* stream) {
    if (const int rc = vit_gemm_check(g, "dtk_vit_gemm", false)) return rc;
    return with_operand_type(g->operand_type == DTK_OPERAND_BF16, [&](auto t) {
        return run_gemm<decltype(t)>(*g, gemm_path(g->D, g->flags), vit_gemm_hidden(g), dtk_stream(stream));
    });
}

// The plan of a role that launch_gemm sends to the RT = 3 form of gemm_ws_kernel (the tests mirror it): the conditions are launch_gemm's.
extern "C" int dtk_vit_gemm_ws_plan(int role, int D, int flags, int64_t rows, int S, int32_t* chunks, int32_t* tpc, int32_t* last) {
    if (!chunks || !tpc || !last || rows <= 0 || (role != DTK_VIT_GEMM_FC1 && role != DTK_VIT_GEMM_QKV)) return 0;
    const int epi = role == DTK_VIT_GEMM_FC1 ? EPI_GELU : EPI_QKV, N = role == DTK_VIT_GEMM_FC1 ? 4 * D : 3 * D;
    if (!gemm_ws96_runs(gemm_path(D, flags), epi, rows, N, D, S, 0)) return 0;
    const Ws96Plan p = gemm_ws96_plan(N, rows);
    const long long tiles = dtk_cdiv(rows, WS_ROWS);
    for (int g = 0; g < p.groups; ++g) {
        chunks[g] = p.chunks[g];
        tpc[g] = p.tpc[g];
        last[g] = (int32_t)(tiles - (long long)(p.chunks[g] - 1) * p.tpc[g]);
    }
    return p.groups;
}

// The same stage on split operands (vit_split.h): hi / lo planes of A, of w_scale * W and of the 16-bit outputs; the residual roles
// add their update to the fp32 stream x.
extern "C" int dtk_vit_gemm_split(const dtk_vit_gemm_args* g, void* stream) {
    if (const int rc = vit_gemm_check(g, "dtk_vit_gemm_split", true)) return rc;
    DTK_REQUIRE(!g->ln_out, "dtk_vit_gemm_split: the split blocks have their own LayerNorm");
    return with_operand_type(g->operand_type == DTK_OPERAND_BF16, [&](auto t) {
        return run_gemm_split<decltype(t)>(*g, gemm_path(g->D, g->flags), vit_gemm_hidden(g), dtk_stream(stream));
    });
}
