/*
 * dtk.h -- C-ABI of libdtk.so: the MI355X (gfx950) device programs behind DINO-Tracker's per-video
 * inference hot path.  Plain pointers and sizes only; every pointer is a DEVICE pointer unless said otherwise.
 *
 * The reference (/root/reference, pure PyTorch) has no FFI of its own: the boundary it exposes is the Python API
 * of models/tracker.py, models/model_inference.py, models/extractor.py.  Each entry point
 * below names the reference call site(s) it replaces (file:line in /root/reference); the Python classes in
 * dino_tracker_amd/ keep the reference's names and signatures and call these through ctypes
 * (INTEGRATION.md shows the binding a reference maintainer would add).
 *
 * Conventions
 *   - return 0 on success, negative DTK_E_* on failure; dtk_last_error() gives a message (thread-local).
 *   - asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream); no host sync inside unless
 *     stated; the caller owns every buffer, nothing is allocated or retained by the library.
 *   - feature volume layout ("token-major"): F[t][cell][c], cell = row*pw + col, c contiguous, fp32.
 *   - pixel coordinates are (x, y) at model resolution; cell (row, col) centre = (stride*col + patch/2,
 *     stride*row + patch/2)  (models/networks/tracker_head.py:72-81).
 */
#ifndef DTK_H_
#define DTK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTK_OK 0
#define DTK_E_INVALID (-1)   /* bad argument / unsupported size */
#define DTK_E_HIP (-2)       /* a HIP runtime call or kernel launch failed */
#define DTK_E_WORKSPACE (-3) /* workspace too small */

/* geometry of one video at model resolution; ph/pw = 1 + (dim - patch) / stride (models/extractor.py:171-181) */
typedef struct dtk_geom {
    int32_t T;        /* frames */
    int32_t C;        /* feature width (384 ViT-S, 768 ViT-B, 1024 ViT-L) */
    int32_t ph, pw;   /* token grid */
    int32_t video_h, video_w;
    int32_t patch, stride;
    float radius;     /* soft-argmax disk radius in px (tracker_head.py:47, 35) */
} dtk_geom;

/* TrackerHead.cnn_refiner parameters AFTER NormalizedConv2d's W / sum(W) (conv_norm.py:34-46), which
 * dtk_head_prepare computes on device.  Layout: w1[16][9], b1[16], w2[16][9] (w2[ch][tap]), b2[1]; tap = 3*ky+kx. */
#define DTK_HEAD_HIDDEN 16
#define DTK_HEAD_PARAMS (16 * 9 + 16 + 16 * 9 + 1)

int dtk_version(void);
const char* dtk_last_error(void);

/* ---- per-kernel timing (used by bench.py for the roofline figures) -----------------------------------------
 * dtk_profile_enable(1) makes every kernel launch of this library be bracketed by hipEvents on its stream;
 * dtk_profile_collect() waits for them and aggregates per kernel name; *_name/_ms/_launches read entry i. */
int dtk_profile_enable(int on);
int dtk_profile_collect(void);
const char* dtk_profile_name(int i);
double dtk_profile_ms(int i);
long long dtk_profile_launches(int i);

/* ---- feature volume ------------------------------------------------------------------------------------ */
/* Reference layout [T][C][ph][pw] (dino_embed_video.pt, models/tracker.py:65-71) -> token-major [T][HW][C]
 * plus per-cell L2 norms [T][HW] (the `.norm(dim=1)` of models/tracker.py:162, hoisted to once per video). */
int dtk_pack_features(const float* chw, float* thwc, float* norms, int T, int C, int HW, void* stream);
/* inverse layout conversion (for callers that read `.refined_features` as T x C x h x w) */
int dtk_unpack_features(const float* thwc, float* chw, int T, int C, int HW, void* stream);
/* norms only (after refinement wrote thwc in place) */
int dtk_feature_norms(const float* thwc, float* norms, int T, int C, int HW, void* stream);

/* ---- P1: DINOv2 ViT encoder as driven by VitExtractor (models/extractor.py:23-150, utils.py:33-72) -----------------
 * Host-side structs of DEVICE pointers.  Matrix weights are 16-bit in nn.Linear layout [out][in], in the model's OPERAND
 * TYPE: IEEE fp16 by default (round 3: the same MFMA rate as bf16 with 8x less operand rounding -- round 2's end-to-end
 * error from the video was the bf16 operands), bf16 with DTK_VIT_BF16; vectors are fp32.
 * Upstream facebookresearch/dinov2 parameter names are given for each field (blocks.{i}.*). */
typedef struct dtk_vit_layer {
    const float *ln1_w, *ln1_b;   /* norm1.weight / .bias */
    const void* qkv_w;            /* attn.qkv.weight  16-bit [3D][D] */
    const float* qkv_b;           /* attn.qkv.bias    [3D] */
    const void* proj_w;           /* attn.proj.weight 16-bit [D][D] */
    const float* proj_b;          /* attn.proj.bias */
    const float* ls1;             /* ls1.gamma */
    const float *ln2_w, *ln2_b;   /* norm2.* */
    const void* fc1_w;            /* mlp.fc1.weight 16-bit [4D][D] */
    const float* fc1_b;
    const void* fc2_w;            /* mlp.fc2.weight 16-bit [D][4D] */
    const float* fc2_b;
    const float* ls2;             /* ls2.gamma */
    /* Round 6 -- the ESCALATED precision of a block (csrc/vit_split.h): when qkv_w_lo is not NULL, this block runs every matrix
     * product on split operands (x = hi + lo, three MFMAs per product, fp32-grade results at ~3x the matrix work): the four
     * `*_w` pointers above are then the HI planes and these the LO planes of  w_scale * W  (lo = T(w_scale W - hi); w_scale a
     * power of two -- 2^8 for fp16 so that the lo halves stay normal numbers, 1 for bf16), all four or none.  Blocks can be
     * escalated individually; a model whose operand type is bf16 keeps 16 significant bits this way at fp32's range. */
    const void *qkv_w_lo, *proj_w_lo, *fc1_w_lo, *fc2_w_lo;
    float w_scale;
} dtk_vit_layer;

typedef struct dtk_vit_model {
    int32_t D, heads;             /* d_head = D / heads must be 64 (ViT-S/B/L/g); D <= 1536 */
    int32_t depth;                /* number of blocks to run = hooked layer + 1 (models/extractor.py:137-150) */
    int32_t patch, stride;        /* 14, 7 (models/extractor.py:41-55) */
    float ln_eps;                 /* 1e-6 */
    int32_t flags;                /* 0 or a combination of the DTK_VIT_* bits below */
    const float* patch_w;         /* patch_embed.proj.weight fp32 [D][3][patch][patch] */
    const float* patch_b;         /* patch_embed.proj.bias */
    const float* cls_pos;         /* cls_token + pos_embed[0]  [D] */
    const float* pos;             /* interpolated patch position encoding [ph*pw][D] (models/extractor.py:57-85) */
    const float* mean_std;        /* ImageNet mean[3], std[3] (utils.py:46) */
    const dtk_vit_layer* layers;  /* HOST array of `depth` entries */
    int32_t frame_batch;          /* frames per pass of the encoder (workspace grows with it: 87 MB per frame at 854 x 476, ViT-S); 0 = the library's default (90) */
    int32_t* overflow;            /* DEVICE word or NULL; OR-ed with 1 when a residual update (projection / MLP output) reached
                                   * the fp16 limit 65504 or is not finite (every token of every frame: the LayerNorm that
                                   * applies the update checks it), with 2 / 4 when a value the QKV / fc1 GEMM STORES (Q after
                                   * its scale, K, V / the MLP hidden AFTER the GELU) did: tracked inside those GEMMs' epilogues for every value of every
                                   * frame (round 5; DTK_VIT_CHECK_RANGE adds a scan of the stored tensors, the tests'
                                   * cross-check).  The caller zeroes it.  fp16 activations
                                   * SATURATE (FP16_OVFL mode) instead of becoming inf; a non-zero word means the features
                                   * are not trustworthy and the model should be run with DTK_VIT_BF16. */
    /* Round 6 -- the multi-layer form of get_feature_from_input (models/extractor.py:142-149: the MEAN over the requested layers of
     * the block outputs) in ONE pass: after every block l with bit l of tap_mask set, tap_out [n][1 + R + ph*pw][D] += tap_scale x (the
     * residual stream after block l).  The caller zeroes tap_out and sets tap_scale = 1 / #layers.  NULL / 0: off. */
    float* tap_out;
    uint64_t tap_mask;
    float tap_scale;
    /* The feed-forward of the blocks.  DTK_VIT_FFN_GELU (0, what a zero-initialised caller gets): fc2(GELU(fc1 x)), hidden = 4 D.
     * DTK_VIT_FFN_SWIGLU (ViT-g/14, upstream vit_giant2 with SwiGLUFFNFused: D = 1536, hidden = 4096):
     *     x1, x2 = w12(x).chunk(2);  y = w3(silu(x1) * x2),   mlp.w12 [2 hidden][D] + bias, mlp.w3 [D][hidden] + bias.
     * dtk_vit_layer.fc2_w / fc2_b are then w3, and fc1_w / fc1_b (and fc1_w_lo) the PACKED w12 / b12: row-interleaved in groups of
     * 32 so that a gate row and its value row fall into the same lane of the GEMM's accumulators --
     *     packed row 64 g + i      = w12 row 32 g + i            (gate,  i = 0 .. 31)
     *     packed row 64 g + 32 + i = w12 row hidden + 32 g + i   (value),            g = 0 .. hidden / 32 - 1
     * (every GEMM form gives a wave 64 consecutive columns as four 16-wide fragments: gate fragments 0, 1 meet value fragments 2, 3).
     * One packed copy serves every kernel form; the epilogue writes hidden [rows][hidden], 128 columns per 256 packed ones, and
     * tracks the fp16 range of what it stores as overflow bit 4.  DTK_VIT_GEMM_WS_V1 / GEMM_WIDE_V1 are refused for such a model. */
    int32_t ffn;
    int32_t hidden;               /* 0 = 4 D (GELU); 4096 for SwiGLU */
    /* DINOv2 with registers (upstream prepare_tokens_with_masks, num_register_tokens = 4 for the hub's dinov2_vit*14_reg): R learned
     * rows between the CLS row and the patch rows, inserted AFTER the position encoding is added (they carry none):
     *     row 0 = cls_pos,  rows 1 .. R = registers[0 .. R-1],  rows 1 + R .. = patch tokens + pos,  S = 1 + R + ph*pw.
     * They attend and are attended to like any token; feat_out drops them together with CLS.  0 (what a zero-initialised caller
     * gets): the plain model.  0 <= n_registers <= 16. */
    int32_t n_registers;
    const float* registers;       /* DEVICE [n_registers][D] fp32 (register_tokens); NULL only with n_registers == 0 */
} dtk_vit_model;
#define DTK_VIT_FFN_GELU 0
#define DTK_VIT_FFN_SWIGLU 1

#define DTK_VIT_TILED_GEMMS 1   /* run the K = 384 GEMMs on the tiled kernel too (cross-check in the tests) */
#define DTK_VIT_BF16 2          /* operand type bf16 instead of fp16 (weights must then be bf16) */
#define DTK_VIT_CHECK_RANGE 4   /* scan Q / K / V^T and the MLP hidden of every block for saturated values (costs a pass) */
/* (8 selected the round-2/3 attention kernel until it left the library: retired, not reused; dtk_vit_forward refuses unknown bits) */
#define DTK_VIT_GEMM_WS_V1 16   /* the K = 384 weight-stationary GEMMs in their round 1-3 form (A / B measurement, cross-check) */
#define DTK_VIT_ATTENTION_V4 32 /* attention on the round-4/5 kernel (one wave per SIMD, 64 queries per wave: csrc/vit_attention4.h) instead of
                                 * round 6's 128 queries per wave (csrc/vit_attention6.h): A / B measurement, cross-check */
#define DTK_VIT_NO_LN_FUSION 128 /* D = 384: keep both LayerNorms launches of their own instead of running LayerNorm-2 inside the attention
                                  * projection's epilogue and the LayerNorm of the next block inside fc2's (A / B measurement, cross-check:
                                  * the results are bit-identical) */
#define DTK_VIT_GEMM_WIDE_V1 64 /* the LDS-DMA GEMMs (256 x 256 tiles of D = 768 / 1024, fc2 of D = 384, the split-operand GEMMs) in their
                                 * round 4-5 form: 8-byte stores straight from the D tiles instead of whole rows through LDS, fragments read
                                 * at the top of every k-step (A / B measurement, cross-check: the results are bit-identical) */
#define DTK_OPERAND_F16 0
#define DTK_OPERAND_BF16 1
#define DTK_OPERAND_ATTENTION_V4 0x2000 /* OR-ed into dtk_vit_attention's operand_type: the same selection as DTK_VIT_ATTENTION_V4 for the
                                         * stand-alone stage; every other bit is refused */

/* frames [n][3][video_h][video_w] fp32 in [0,1] -> block output of layer depth-1 (before the final norm):
 * With R = n_registers (0 for the plain models):
 * tokens_out [n][1 + R + ph*pw][D] (CLS first, then the registers, then the patches; what get_feature_from_input returns) and/or
 * feat_out   [n][ph*pw][D]     (CLS and the registers dropped: the token-major feature volume of this library) and/or
 * qkv_out    [n][1 + R + ph*pw][3D] the output of blocks[depth-1].attn.qkv (the tensor the reference's qkv hook records,
 *            models/extractor.py:107-118; the key / query / value facets are reshapes of it, :245-267).
 * Any of them may be NULL (not all). */
size_t dtk_vit_workspace_bytes(const dtk_vit_model* m, int video_h, int video_w, int frames);
int dtk_vit_forward(const dtk_vit_model* m, const float* frames, int nframes, int video_h, int video_w,
                    float* tokens_out, float* feat_out, float* qkv_out, void* workspace, size_t workspace_bytes,
                    void* stream);

/* The multi-head self-attention stage of a block on its own, d_head = 64 (what runs between the QKV and the projection
 * GEMMs inside dtk_vit_forward; upstream Attention.forward, hooked by models/extractor.py:101-104).  Operands in
 * `operand_type` (DTK_OPERAND_F16 / DTK_OPERAND_BF16):
 *   q  [frames][heads][Sp][64]   queries, ALREADY multiplied by log2(e) / sqrt(64) (the softmax runs in the exp2 domain)
 *   k  [frames][heads][Sp][64]   keys; rows S .. Sp-1 must be finite (zero)
 *   vt [frames][heads][64][Sp]   values, transposed; columns S .. Sp-1 must be finite (zero)
 *   out[frames][S][heads*64]     softmax(q k^T) v, heads concatenated (the input of attn.proj)
 * Sp = S rounded up to a multiple of 64 (dtk_vit_forward uses 128). */
int dtk_vit_attention(const void* q, const void* k, const void* vt, void* out, int frames, int heads, int S, int Sp,
                      int operand_type, void* stream);
/* The same stage on SPLIT operands (the escalated precision of a block, dtk_vit_layer.qkv_w_lo): every tensor as hi / lo planes
 * of `operand_type` in the layouts above (x = hi + lo); scores, probabilities and both products carry ~22 (fp16) / ~16 (bf16)
 * significant bits. */
int dtk_vit_attention_split(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* vt_hi,
                            const void* vt_lo, void* out_hi, void* out_lo, int frames, int heads, int S, int Sp, int operand_type,
                            void* stream);

/* ONE GEMM of a block on its own: C = A W^T with the epilogue of its role, on exactly the kernel dtk_vit_forward runs for a model
 * of width D (384, 768, 1024 or 1536) with the DTK_VIT_* bits `flags` (the GEMM bits: TILED_GEMMS, GEMM_WS_V1, GEMM_WIDE_V1,
 * NO_LN_FUSION).  The role fixes N x K and what is written:
 *   DTK_VIT_GEMM_QKV        3D x D    q / k [rows / S][D / 64][Sp][64], vt [rows / S][D / 64][64][Sp]; q scaled by log2(e) / 8.  rows is a
 *                                     multiple of S; the caller zeroes the padding s >= S (dtk_vit_forward does), it is not written
 *   DTK_VIT_GEMM_QKV_FACET  3D x D    out_f32 [rows][3D] = A W^T + bias
 *   DTK_VIT_GEMM_PROJ       D x D     out [rows][D] = gamma * (A W^T + bias), 16-bit (the pending residual update).  With ln_out set: as
 *                                     FC2 below, where dtk_vit_forward fuses the block's LayerNorm-2 (D = 384, none of TILED_GEMMS /
 *                                     GEMM_WS_V1 / GEMM_WIDE_V1 / NO_LN_FUSION)
 *   DTK_VIT_GEMM_FC1        4D x D    out [rows][4D] = GELU(A W^T + bias), 16-bit
 *   DTK_VIT_GEMM_FC2        D x 4D    as PROJ.  With ln_out set (D = 384, none of TILED_GEMMS / GEMM_WIDE_V1 / NO_LN_FUSION: where
 *                                     dtk_vit_forward fuses it) the update is NOT stored: ln_x [rows][D] += it and ln_out [rows][D] =
 *                                     LayerNorm(ln_x; ln_w, ln_b, ln_eps), 16-bit
 *   DTK_VIT_GEMM_FC1_SWIGLU 8192 x 1536  D = 1536 only: w = the PACKED w12 (dtk_vit_model.ffn), bias the packed b12;
 *                                     out [rows][4096] = silu(gate) * value, 16-bit (split: out, out_lo); ovf bit 4.  Refused with
 *                                     GEMM_WS_V1 / GEMM_WIDE_V1 in flags
 *   DTK_VIT_GEMM_FC2_SWIGLU 1536 x 4096  D = 1536 only: w3, otherwise as FC2 (no fused LayerNorm at this width)
 * a [rows][K] and w [N][K] are 16-bit in `operand_type`, bias / gamma fp32 [N].  ovf: optional device word, OR-ed with 2 (QKV) / 4
 * (FC1) when a stored value reaches the fp16 limit and with 1 by the fused LayerNorm (fp16 operands only; the caller zeroes it).
 * dtk_vit_gemm_split: the same roles on hi / lo planes (a, a_lo; w, w_lo = planes of w_scale * W; q .. vt_lo; out, out_lo); PROJ and
 * FC2 add gamma * (A W^T + bias) to the fp32 stream x [rows][D] instead of storing an update. */
#define DTK_VIT_GEMM_QKV 0
#define DTK_VIT_GEMM_QKV_FACET 1
#define DTK_VIT_GEMM_PROJ 2
#define DTK_VIT_GEMM_FC1 3
#define DTK_VIT_GEMM_FC2 4
#define DTK_VIT_GEMM_FC1_SWIGLU 5
#define DTK_VIT_GEMM_FC2_SWIGLU 6
typedef struct dtk_vit_gemm_args {
    int32_t role, D, flags, operand_type;
    int64_t rows;
    int32_t S, Sp;
    float ln_eps, w_scale;
    const void *a, *a_lo, *w, *w_lo;
    const float *bias, *gamma;
    void *q, *k, *vt, *q_lo, *k_lo, *vt_lo;
    void *out, *out_lo;
    float *out_f32, *x, *ln_x;
    const float *ln_w, *ln_b;
    void* ln_out;
    int32_t* ovf;
} dtk_vit_gemm_args;
int dtk_vit_gemm(const dtk_vit_gemm_args* g, void* stream);
int dtk_vit_gemm_split(const dtk_vit_gemm_args* g, void* stream);
/* How dtk_vit_gemm / dtk_vit_forward lay a role's launch out when it runs the 96-features-per-wave weight-stationary kernel (D = 384,
 * roles FC1 and QKV without TILED_GEMMS / GEMM_WS_V1; S = tokens per frame, used by QKV only: several frames shorter than 32 rows
 * run another kernel): returns the number of 384-column groups, 0 when the role does not run that kernel under these flags.  Group g
 * runs as chunks[g] workgroups of tpc[g] consecutive 32-row token tiles, the last of them with last[g] tiles; the arrays hold four
 * entries.  Host arithmetic only: no device is touched. */
int dtk_vit_gemm_ws_plan(int role, int D, int flags, int64_t rows, int S, int32_t* chunks, int32_t* tpc, int32_t* last);

/* ---- P2: Delta-DINO refinement (models/tracker.py:113-135; models/networks/delta_dino.py:53-61;
 *      models/utils.py:7-45), fp32-grade on the fp16 MFMA (operands split into hi + lo halves, 3 products) ----------
 * dtk_delta_dino_pack: layer l in 0..3 (state-dict keys layers.{4l}.{weight,bias} = conv [Cout][Cin][5][5] and
 *   layers.{4l+1}.{weight,bias,running_mean,running_var} = BatchNorm2d, eval mode) -> kernel layout
 *   packed = Wk[25][CinP][CoutP] | scale[CoutP] | shift[CoutP] | split-fp16 weight planes (hi, lo; 2^8 w) in the
 *   tile order of the convolution kernels  (dtk_delta_dino_packed_floats floats in total; opaque to the caller).
 * dtk_delta_dino_refine: for frames t0 .. t0+nframes-1: out[t] = dino[t] + align(CNN(video[t])), token-major, plus
 *   per-cell norms (may be NULL).  video is [T][3][video_h][video_w] fp32 in [0,1] (data/data_utils.py:79-104),
 *   packed = 4 device pointers (host array).  BlurPool = antialiased_cnns.BlurPool(stride 2): reflect-pad (1,2,1,2),
 *   4x4 binomial. */
size_t dtk_delta_dino_packed_floats(int layer, int C);
int dtk_delta_dino_pack(int layer, int C, const float* w, const float* bias, const float* bn_w, const float* bn_b,
                        const float* bn_mean, const float* bn_var, float eps, float* packed, void* stream);
size_t dtk_delta_dino_workspace_bytes(const dtk_geom* g);
int dtk_delta_dino_refine(const dtk_geom* g, const float* video, const float* dino, const float* const* packed,
                          float* out, float* norms, int t0, int nframes, void* workspace, size_t workspace_bytes,
                          void* stream);
/* The same with the operand precision of the 5x5 convolutions of layers 2-4 chosen by the caller:
 *   DTK_DD_SPLIT  every fp32 operand as hi + lo fp16 halves, three MFMA products per term (fp32-grade: 3e-5 of the reference)
 *   DTK_DD_FP16   the hi halves only: plain fp16 operands, fp32 accumulation, one product per term.  The first layer, its
 *                 BatchNorm + ReLU and the first blur-pool are ONE kernel (conv1_pool_half_kernel): the full-resolution
 *                 64-channel activation is never written.  Layers 2-4 run on conv5x5_half_kernel (conflict-free LDS
 *                 fragment reads, channel-pair stores: 4 bytes per lane in fp16, 8 in fp32).
 *   DTK_DD_FP16_V1  the same values, bit for bit, from the kernel sequence DTK_DD_FP16 ran before those two kernels
 *                 (conv1_split_kernel<true> + blurpool_half_kernel, conv5x5_split_kernel<.., SINGLE>): the A / B switch and the
 *                 reference of tests/test_gpu_p2_fp16_fused.py.
 * DEFAULTS DIFFER BY ENTRY POINT, on purpose: dtk_delta_dino_refine (above, the round 1-3 entry) always means DTK_DD_SPLIT, so a
 * C caller that never heard of the mode keeps the fp32-grade result; the Python mirror (dino_tracker_amd/delta_dino.py) calls
 * THIS entry and defaults to DTK_DD_FP16 since round 4 (the end-to-end position error is unchanged to 1e-5 px behind the fp16
 * ViT operands, profiles/r04_e2e_error_p2_operands.json; DTK_P2_OPERANDS=split or DeltaDINO.conv_operands = "split" restores the
 * other).  tests/test_gpu_p2.py pins both modes against the reference-written golden, each with its own tolerance. */
#define DTK_DD_SPLIT 0
#define DTK_DD_FP16 1
#define DTK_DD_FP16_V1 2
int dtk_delta_dino_refine_mode(const dtk_geom* g, const float* video, const float* dino, const float* const* packed,
                               float* out, float* norms, int t0, int nframes, int operands, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---- K8: bilinear point sampling -------------------------------------------------------------------------
 * Tracker.sample_embeddings (models/tracker.py:96-111 -> utils.py:75-101) for integral frame indices:
 * out[b][:] = bilinear(F[t_idx[b]], (xy[b] - patch/2) / stride), border clamp, align_corners.
 * out row b is written at out + out_row[b]*C if out_row != NULL else out + b*C. */
int dtk_sample_points(const dtk_geom* g, const float* feat, const float* xy, const int32_t* t_idx,
                      const int32_t* out_row, float* out, int B, void* stream);

/* Literal utils.bilinear_interpolate_video (utils.py:75-101; what Tracker.sample_embeddings calls, models/tracker.py:96-111)
 * on a token-major volume feat[T][ph*pw][C]: pts[B][3] = (x, y, t) ALREADY in [-1, 1] (grid_sample coordinates),
 * trilinear, align_corners=True, border padding -> out[B][C].  No patch / stride enters. */
int dtk_sample_grid(const float* feat, int T, int C, int ph, int pw, const float* pts, float* out, int B, void* stream);

/* ---- TrackerHead parameters ---------------------------------------------------------------------------- */
/* raw state-dict tensors (cnn_refiner.0.weight [16,1,3,3], .0.bias [16], .2.weight [1,16,3,3], .2.bias [1])
 * -> normalised packed parameters head[DTK_HEAD_PARAMS] (conv_norm.py:34-46). */
int dtk_head_prepare(const float* w1, const float* b1, const float* w2, const float* b2, float* head, void* stream);

/* TrackerHead.forward alone (models/networks/tracker_head.py:107-121) on B ReLU'd cost volumes maps[B][ph*pw]:
 * out[b] = normalised (x, y) in [-1,1] (normalized != 0) or pixels. */
int dtk_head_forward(const dtk_geom* g, const float* head, const float* maps, float* out_xy, int B, int normalized,
                     void* stream);

/* TrackerHead.forward / backward of the TRAINING step (tracker_head.py:68-121 under autograd).  `head` = the packed parameters of
 * dtk_head_prepare (305 floats: w1[16][9] | b1[16] | w2[16][9] | b2, weights already normalised W / sum W).
 * dtk_head_forward_train = dtk_head_forward + stats[b][4] = (arg-max cell as int bits, softmax maximum, partition sum, disk
 * mass before the zero-mass fallback).  dtk_head_backward: grad_out[b][2] -> dmaps[b][ph*pw] (gradient with respect to the
 * input maps; the caller ZEROES it: only the 15 x 15 window around each arg-max is written) and dhead_partial[b][305] (per-map
 * parameter gradients, same packing; the caller sums over b).  Exact when no map's fallback fired (stats[b][3] >= 1e-8): then
 * the output does not depend on logits outside the disk and the backward is local to the window; the caller must take another
 * route for a batch in which a fallback fired.  Needs radius / stride <= 5. */
int dtk_head_forward_train(const dtk_geom* g, const float* head, const float* maps, float* out_xy, float* stats, int B,
                           int normalized, void* stream);
int dtk_head_backward(const dtk_geom* g, const float* head, const float* maps, const float* stats, const float* grad_out,
                      float* dmaps, float* dhead_partial, int B, int normalized, void* stream);

/* The split-fp16 implicit-GEMM 5 x 5 convolution as a stand-alone operator: forward and data gradient of the Delta-DINO layers
 * in the TRAINING step (models/networks/delta_dino.py:29-44 under autograd), fp32-grade (operands as hi + lo fp16 planes, three
 * matrix-core products per term), stride 1, "same" size, dilation 1 or 2, reflect or zero padding.  Cin a multiple of 16.
 *   dtk_conv_split_pack     w [Cout][Cin][5][5] -> the kernel's weight planes (dtk_conv_split_weight_halves(Cin, Cout) fp16 values
 *                           each).  flip_transpose: w is [Cin][Cout][5][5] and taps are read reversed -- the operator of the data
 *                           gradient with respect to the forward's input.
 *   dtk_conv_split_input    x [N][C][H][W] fp32 times *scale (device scalar or NULL) -> hi / lo planes [N][H+2b][W+2b][C] with a
 *                           ring of b zero pixels.  C a multiple of 8.
 *   dtk_conv_split_run      planes [N][H][W][Cin] -> out [N][H][W][Cout] fp32.  fp16_only: use the hi halves only (plain fp16
 *                           operands, 2^-11 relative per operand, a third of the matrix-core work) -- the "fp16" training mode; the
 *                           same switch exists on dtk_conv_wgrad_split.
 *   dtk_conv_split_output   y [N][H+2b][W+2b][C] -> [N][C][H][W] divided by *scale; reflect_fold adds the ring back onto the image
 *                           with the adjoint of the reflect padding (b = 2 * dilation: the data gradient of a reflect-padded
 *                           convolution is the zero-padded convolution of dY over the padded domain, folded). */
size_t dtk_conv_split_weight_halves(int Cin, int Cout);
int dtk_conv_split_pack(const float* w, int Cin, int Cout, int flip_transpose, void* Wh, void* Wl, void* stream);
int dtk_conv_split_input(const float* x, int N, int C, int H, int W, int border, const float* scale, void* hi, void* lo,
                         void* stream);
int dtk_conv_split_run(const void* in_hi, const void* in_lo, const void* Wh, const void* Wl, float* out_nhwc, int N, int H, int W,
                       int Cin, int Cout, int dilation, int zero_pad, int fp16_only, void* stream);
int dtk_conv_split_output(const float* y_nhwc, int N, int C, int H, int W, int border, int reflect_fold, const float* scale,
                          float* out_nchw, void* stream);

/* Weight gradient of the same convolution without an unfolded operand: dw [Cout][Cin][5][5] (overwritten) = sum over frames and
 * pixels of dy [N][Cout][H][W] (times *scale_dy, a power of two, undone on output) and the padded x [N][Cin][H][W]; both operands
 * fp32 NCHW as autograd holds them, split into fp16 halves while staged (fp32-grade).  workspace: the per-workgroup partial sums
 * (dtk_conv_wgrad_split_workspace_bytes), reduced by a second kernel -- no atomics, deterministic. */
size_t dtk_conv_wgrad_split_workspace_bytes(int N, int Cin, int Cout, int H, int W, int dilation);
int dtk_conv_wgrad_split(const float* x, const float* dy, float* dw, int N, int Cin, int Cout, int H, int W, int dilation,
                         int reflect_pad, const float* scale_dy, int fp16_only, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The contrastive (InfoNCE) terms of the training loss (dino_tracker.py:141-243, :327-343) without the affinity tensors:
 * problem q < Q = B anchor embeddings a[q][i][C] against all n cells of frame fidx[q] of fe[F][C][n]:
 *     s[i][j] = cos(a_i, f_j) (clamped at 1e-8 like the reference),   lse[q][i] = log sum_j exp(s[i][j] / temp)
 * so that the reference's term -log(exp(cos(a_i, b_i) / temp) / sum_j exp(s[i][j] / temp)) = lse - cos(a_i, b_i) / temp.
 * forward writes lse and keeps for backward: nf[F][n] = |f_j|, na[Q][B] = |a_i|, S[Q][B][np] = the cosines (np = n rounded up
 * to a multiple of 4); fet [F][n][C] is scratch.  backward: g[Q][B] = dL/dlse -> da[Q][B][C] (written) and dfe[F][C][n]
 * (ZEROED and written: the sum over the problems of each frame; float atomics, so the last bits depend on the order). */
size_t dtk_contrastive_workspace_bytes(int Q, int B, int C, int n);
int dtk_contrastive_forward(const float* fe, const float* a, const int32_t* fidx, float temp, int Q, int B, int C, int n, int F,
                            float* fet, float* nf, float* na, float* S, float* lse, void* stream);
int dtk_contrastive_backward(const float* fe, const float* a, const int32_t* fidx, float temp, int Q, int B, int C, int n, int F,
                             const float* nf, const float* na, const float* S, const float* lse, const float* g, float* da,
                             float* dfe, void* workspace, size_t workspace_bytes, void* stream);

/* The embedding regularisers of the training loss (dino_tracker.py:128-139): out2 = (mean | |x| / |raw| - 1 |, mean | cos(x, raw) - 1 |)
 * over the F * n cells of x, raw [F][C][n]; cell_sums [3][F * n] keeps the per-cell sums for dtk_emb_reg_backward, which writes
 * dx [F][C][n] for the upstream gradients grad_out2 (device, two floats). */
int dtk_emb_reg_forward(const float* x, const float* raw, int F, int C, int n, float* cell_sums, float* out2, void* stream);
int dtk_emb_reg_backward(const float* x, const float* raw, const float* cell_sums, const float* grad_out2, int F, int C, int n,
                         float* dx, void* stream);

/* Backward of the cosine maps (models/tracker.py:158-173 under autograd) behind dtk_head_backward: maps[b] = relu'd cosine map
 * of emb[b] against frame tgt[b] (dtk_corr_maps with relu = 1), dmaps[b] its gradient (non-zero only on the 15 x 15 window around
 * the arg-max cell stats[b][0], as dtk_head_backward leaves it).  demb[b][C] is written; dfeat[T][ph*pw][C] (token-major, ZEROED
 * by the caller) receives atomic adds.  C <= 1024. */
int dtk_corr_window_backward(const dtk_geom* g, const float* feat, const float* norms, const float* emb, const int32_t* tgt,
                             const float* maps, const float* dmaps, const float* stats, float* demb, float* dfeat, int B,
                             void* stream);

/* NormalizedConv2d.forward as a stand-alone layer (models/networks/conv_norm.py:34-46): x[B][Cin][H][W],
 * w[Cout][Cin][k][k] (RAW weights: the per-kernel W / sum(W) is applied inside), bias[Cout] or NULL -> y[B][Cout][H][W];
 * stride 1, zero padding k/2, k odd.  (The tracker path runs these layers fused inside dtk_track / dtk_head_forward.) */
int dtk_normalized_conv2d(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int H,
                          int W, int k, void* stream);

/* Tracker.get_corr_maps_for_frame_set (models/tracker.py:158-169): cosine maps of M sources against their target
 * frames, maps[m][ph*pw] fp32; relu != 0 applies cmap_relu (:173).  snorm_scratch: M floats. */
int dtk_corr_maps(const dtk_geom* g, const float* feat, const float* norms, const float* emb, const int32_t* src_row,
                  const int32_t* tgt, float* maps, float* snorm_scratch, int M, int relu, void* stream);

/* ---- K9-K13: track sources into target frames ------------------------------------------------------------
 * For each source m < M:  s = emb[src_row[m]] (row of an [R][C] fp32 matrix), a = tgt[m]:
 *   rho = relu(cos(s, F[a](:, r, c)))                     models/tracker.py:158-173
 *   (x, y) = TrackerHead(rho)                             models/networks/tracker_head.py:107-121
 * and out_xy[out_idx[m]] = (x, y) in PIXELS (model_inference.py:52 already applied), or normalised to [-1,1]
 * if normalized != 0 (the value Tracker.forward returns, tracker.py:303-325).
 * src_row / out_idx may be NULL (identity).  Any order of tgt is correct; sources sorted by tgt run fastest.
 * opts->method: DTK_TRACK_EXACT = fp32 everywhere (correlation volume staged through `workspace`), fully asynchronous;
 *               DTK_TRACK_MFMA  = fp16-MFMA correlation reduced on chip to peak records + fp32 window refinement.
 *                 Three tiers decide a source: (1) the no-fallback certificate, (2) whole-map
 *                 refiner statistics on the matrix cores for uncertified sources, (3) the exact path for sources the
 *                 fp16 pass cannot decide.  The sizes of tiers 2 and 3 are read back: this method SYNCHRONISES
 *                 `stream` once per call (twice if tier 2 ran; once more if `dM` is given).
 * opts->normalized: 0 = pixels, 1 = [-1,1].
 * opts->round_sources: sources per round of the MFMA pipeline (0 = default 4 194 304; rounded up to a multiple of 256).
 *                 The workspace size follows it.  Results do not depend on it (tests run several rounds with it).
 * opts->tier: DTK_TIER_AUTO, or DTK_TIER_WHOLE_MAP = skip the certificate, every source takes tier 2 (tests).
 * `dM` (device int32*, may be NULL): if given, the number of sources is min(M, *dM).
 * Token grid: both methods (and dtk_head_forward / dtk_head_forward_train) keep one map's logits and a ring of hidden rows in LDS,
 *                 so they serve grids with  ph * pw + 64 * pw + 16 <= 40 960  floats (160 KiB) -- 101 x 181 (720 x 1280) and
 *                 128 x 128 are inside, 153 x 273 (1080 x 1920) is not -- and return DTK_E_INVALID with a message beyond, before
 *                 any source is processed.  (Up to 2 * ph * pw + 128 * pw + 16 <= 40 960 the map itself sits in LDS as well.)
 * `stats` (HOST pointer, may be NULL): filled before returning; nothing is retained by the library between calls. */
#define DTK_TRACK_EXACT 0
#define DTK_TRACK_MFMA 1
#define DTK_TIER_AUTO 0
#define DTK_TIER_WHOLE_MAP 1
typedef struct dtk_track_opts {
    int32_t method, normalized, round_sources, tier;
    int32_t emb_rows;        /* number of rows of `emb` when sources go through src_row (0 = unknown): lets DTK_TRACK_MFMA convert
                              * the rows once per call instead of every round's sources */
} dtk_track_opts;
typedef struct dtk_track_stats {
    int32_t sources;         /* sources processed (min(M, *dM)) */
    int32_t whole_map_tier;  /* of which decided with whole-map statistics (tier 2) */
    int32_t exact_tier;      /* of which re-done on the exact fp32 path (tier 3) */
    int32_t syncs;           /* host synchronisations of `stream` this call made */
} dtk_track_stats;
size_t dtk_track_workspace_bytes(const dtk_geom* g, int M, const dtk_track_opts* opts);
int dtk_track(const dtk_geom* g, const float* feat, const float* norms, const void* feat_f16,
              const float* head, const float* emb, const int32_t* src_row, const int32_t* tgt,
              const int32_t* out_idx, float* out_xy, int M, const int32_t* dM, const dtk_track_opts* opts,
              dtk_track_stats* stats, void* workspace, size_t workspace_bytes, void* stream);

/* Arg-max cell of the RAW cosine map of each source against its target frame, and the cosine there: row arg-max of
 * the affinity matrix of the best-buddies preprocessing (preprocessing_dino_bb/extract_dino_best_buddies.py:36-39;
 * torch.argmax semantics: first maximum).  Sources are rows of `emb` like in dtk_track (src_row may be NULL); results go to
 * arg_cell[m], arg_cos[m].  DTK_TRACK_MFMA = fp16 candidate search + fp32 re-scoring, undecidable sources on the exact path
 * (one stream synchronisation); DTK_TRACK_EXACT = fp32 everywhere.  Workspace: dtk_track_workspace_bytes of the method. */
int dtk_argmax_cells(const dtk_geom* g, const float* feat, const float* norms, const void* feat_f16, const float* emb,
                     const int32_t* src_row, const int32_t* tgt, int32_t* arg_cell, float* arg_cos, int M, int method,
                     void* workspace, size_t workspace_bytes, void* stream);

/* DINO best-buddy ambiguity ratio (preprocessing_dino_bb/compute_dino_bb_nms.py:12-66): for each source m
 * (row src_row[m] of emb = the feature of a best-buddy cell) the cosine affinity row against frame tgt[m], its top-`topk`
 * entries (:14), boxes of +-box_size px around their cell centres (:21-27), torchvision batched_nms at iou_thresh (:30),
 * suppressed affinities zeroed (:34-36), then the two largest of the masked list -> peak_affs[m][0..1] (:38) and
 * r[m] = second / first (:42).  fp32 everywhere (exact-path correlation).  Workspace: dtk_bb_nms_workspace_bytes. */
size_t dtk_bb_nms_workspace_bytes(const dtk_geom* g, int M);
int dtk_bb_nms(const dtk_geom* g, const float* feat, const float* norms, const float* emb, const int32_t* src_row,
               const int32_t* tgt, float box_size, float iou_thresh, int topk, float* peak_affs, float* r, int M,
               void* workspace, size_t workspace_bytes, void* stream);

/* ---- optical-flow trajectory preprocessing (SURVEY 8f N1 inputs) --------------------------------------------------------
 * Trajectories traj [N][T][2] fp32 (x, y), NaN where a point is not tracked (untracked = either coordinate NaN).
 *
 * fg / bg split (preprocessing/split_trajectories_to_fg_bg.py:61-67): per row n the first frame s with a tracked point,
 * the point rounded half-to-even (torch.round), fg[n] = masks[s][y][x] > 0 (masks [Tm][H][W] uint8).  Rows with no tracked
 * frame, or whose start point rounds outside the mask (or s >= Tm), get fg[n] = 0 and are counted in *err (device int32,
 * zeroed by the call): the reference would index with NaN-cast or wrapping indices there. */
int dtk_traj_start_fg(const float* traj, int N, int T, const uint8_t* masks, int Tm, int H, int W, uint8_t* fg, int32_t* err,
                      void* stream);

/* Nearest trajectory of every token-grid point in every frame (preprocessing_dino_bb/of_filter_dino_best_buddies.py:9-29,
 * :50-54): grid point g = (origin + stride * (g % gw), origin + stride * (g / gw)) -- dino_bb_utils.create_meshgrid with
 * origin = patch / 2 --, idx[t][g] = argmin over n of |traj[n][t] - g| compared as (d^2 in fp32, n) lexicographically: the
 * lowest n on equal distances (torch's first-index rule), untracked points = +inf, 0 when frame t has no tracked point.
 * Workspace: dtk_nearest_traj_workspace_bytes (the compacted tracked points of every frame, worst case N per frame). */
size_t dtk_nearest_traj_workspace_bytes(int N, int T, int gh, int gw);
int dtk_nearest_traj(const float* traj, int N, int T, int gh, int gw, float origin, float stride, int32_t* idx,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Optical-flow filter of the best buddies of all frame pairs in one call (of_filter_dino_best_buddies.py:83-94).  Pair p is
 * frames (pair_st[2p], pair_st[2p+1]) = (s, t) with entries pair_off[p] .. pair_off[p+1] of src / tgt ([M][2] pixel (x, y)).
 * cell = ((xy - origin) // stride) (torch float floor division), ns = idx[s][cell(src)], nt = idx[t][cell(tgt)] (idx from
 * dtk_nearest_traj on the same grid), keep[e] = traj[ns][t] untracked AND traj[nt][s] untracked -- the reference's sense: it
 * keeps the buddies whose flow trajectory is lost.  Entries whose cell lies outside the grid (or whose frames are outside
 * [0, T)) get keep 0 and are counted in *err (device int32, zeroed by the call). */
int dtk_of_filter_keep(const float* traj, int N, int T, const int32_t* idx, int gh, int gw, float origin, float stride,
                       const float* src, const float* tgt, const int32_t* pair_off, const int32_t* pair_st, int P,
                       uint8_t* keep, int32_t* err, void* stream);

/* 16-bit copies of the feature volume consumed by DTK_TRACK_MFMA (C % 32 == 0), one buffer of dtk_feat_f16_bytes(g):
 *   - f16[t][row][col][c] = 32 F/|F|, every map row padded with zero cells to a multiple of 128 columns (an N-tile of the
 *     candidate GEMM is one map row);
 *   - at C = 384, behind it (256-byte aligned): the split planes of the window correlation, [t][cell][chunk of 32
 *     channels][hi 32 | lo 32] with s F = hi + lo (fp16 both) -- T*ph*pw*C*4 more bytes, made once per volume instead of
 *     once per staged element of every window box;
 *   - behind that (256-byte aligned), a 256-byte slot whose first float is s: 2^5, or the largest power of two with
 *     s * (largest cell norm of the volume) <= 2^14 when the features are large (round 6: DINOv2-like outlier statistics put
 *     components beyond 2047 = 65504 / 32) -- chosen on the device by dtk_make_feat_f16, read by the window-correlation kernels. */
size_t dtk_feat_f16_bytes(const dtk_geom* g);
int dtk_make_feat_f16(const dtk_geom* g, const float* feat, const float* norms, void* feat_f16, void* stream);

/* ---- K14: cosine similarity along trajectories -----------------------------------------------------------
 * ModelInference.compute_trajectory_cos_sims (models/model_inference.py:110-126):
 * cs[n][t] = cos(S[n][tq[n]], S[n][t]) with F.cosine_similarity semantics (eps 1e-8). S is [N][T][C]. */
int dtk_traj_cos_sims(const float* S, const int32_t* tq, float* cs, int N, int T, int C, void* stream);

/* ---- anchor bookkeeping (models/model_inference.py:156-165) ---------------------------------------------
 * From cs [N][T] and the anchor threshold build, on device and without host sync:
 *   n_anchors[N], pair_off[N+1] (pairs in n-major order, pair p of query n with its k-th anchor = pair_off[n]+k),
 *   and the source lists of the anchor stage sorted by anchor frame:
 *   src_row[m] = n*T + t, tgt[m] = a, out_idx[m] = p*T + t, for m < M_total = P*T (P = pair_off[N]).
 * counts[0] = P, counts[1] = M_total, counts[2] = number of queries with zero anchors (counts has 4 entries).
 * pair_frame must hold N*T entries, the three lists N*T*T entries (worst case), scratch 2*T+2 entries. */
int dtk_build_anchor_sources(const float* cs, float anchor_th, int N, int T, int32_t* n_anchors, int32_t* pair_off,
                             int32_t* pair_frame, int32_t* src_row, int32_t* tgt, int32_t* out_idx,
                             int32_t* counts, int32_t* scratch, void* stream);

/* The anchor stage restricted to the maps the occlusion flags depend on (what ModelInference.infer runs).  With
 *   anchor(n,t) = cs >= anchor_th,  low(n,t) = cs < cos_th,  undecided = !anchor && !low  (a NaN cs is undecided),
 *   needed(n,t) = anchor || undecided,  query n OPEN = it has >= 1 anchor and >= 1 undecided frame,
 * occ[n][t] = med > tau || low with tau = max of med over the anchor frames: an anchor frame has occ = low, a low frame
 * occ = 1, so green[p][t] matters only for the pairs p of open queries at their needed columns t.  Exact, no approximation.
 * n_anchors, pair_off, pair_frame, counts[0] (= P, ALL anchor pairs), counts[2] and the [P][T][2] layout of green are those
 * of dtk_build_anchor_sources; the source lists hold (open n, anchor a of n, needed column t of n) only, sorted by a, within
 * a by n, within a pair by t: src_row = n*T + t, tgt = a, out_idx = p*T + t.  counts[1] = emitted sources (the valid prefix
 * of the three lists; nothing is written behind it), counts[3] = open queries.  No host sync.  Buffer sizes as above, except
 * scratch: 2*T + 2 + N entries (N more: the per-query source count). */
int dtk_build_anchor_sources_needed(const float* cs, float anchor_th, float cos_th, int N, int T, int32_t* n_anchors,
                                    int32_t* pair_off, int32_t* pair_frame, int32_t* src_row, int32_t* tgt, int32_t* out_idx,
                                    int32_t* counts, int32_t* scratch, void* stream);

/* ---- K15: occlusion (models/model_inference.py:169-200) ---------------------------------------------------
 * green [P][T][2] (anchor trajectories, pair-major), pair_off [N+1], pair_frame [P] (anchor frame of pair p),
 * traj [N][T][2], cs [N][T]  ->  occ [N][T] (uint8 0/1). */
int dtk_occlusion(const float* green, const int32_t* pair_off, const int32_t* pair_frame, const float* traj,
                  const float* cs, float anchor_th, float cos_th, uint8_t* occ, int N, int T, void* stream);

/* The same flags from a green that holds only what dtk_build_anchor_sources_needed listed (same thresholds): green[p][t] is
 * read for the pairs of open queries at their needed columns and nowhere else (the rest may be uninitialised memory);
 * distances, ranks and medians are computed only there; the other frames get low(n,t), a query without anchors all ones. */
int dtk_occlusion_needed(const float* green, const int32_t* pair_off, const int32_t* pair_frame, const float* traj,
                         const float* cs, float anchor_th, float cos_th, uint8_t* occ, int N, int T, void* stream);

/* ---- TAP-Vid metric counts (eval/metrics.py:7-147 for one video) ----------------------------------
 * pred_tracks / gt_tracks [N][T][2] f32 (x, y), *_occluded [N][T] (uint8 0/1), query_frame [N]; coordinates are scaled
 * to the 256 x 256 evaluation raster by the four factors first (eval/metrics.py:204-211).  first_mode = 0: 'strided'
 * queries (every frame but the query frame is evaluated), 1: 'first'.  counts18 (device, uint64):
 * [0] evaluated, [1] occlusion agreements, [2] visible, then for thresholds 1, 2, 4, 8, 16 px:
 * [3+3i] within & visible, [4+3i] true positives, [5+3i] false positives.  The host turns them into
 * occlusion_accuracy, pts_within_*, jaccard_* and their averages (dino_tracker_amd/tapvid.py). */
int dtk_tapvid_counts(const float* pred_tracks, const uint8_t* pred_occluded, const float* gt_tracks,
                      const uint8_t* gt_occluded, const int32_t* query_frame, float pred_scale_x, float pred_scale_y,
                      float gt_scale_x, float gt_scale_y, int first_mode, int N, int T, unsigned long long* counts18,
                      void* stream);

/* ---- BADJA metric counts (eval/metrics.py:226-287, compute_badja_metrics_for_video for one video) ------------------
 * pred_tracks [N][T][2] f32 (x, y), scaled in float32 by the two factors first (metrics.py:266-267); gt_tracks [N][T][2]
 * f64, as the benchmark pickle holds them; gt_occluded [N][T] uint8 (0 = visible); segmentations [T_seg][H][W], uint8
 * (seg_is_float = 0) or f32 (1), 1 <= T_seg <= T.  area[t] = number of pixels > 0 (integer reduction into `areas`
 * [T_seg] uint64, device, overwritten); thr[t] = float32(0.2) sqrtf(float32(area[t])).  For every point and every t in
 * 1 .. T_seg - 1 that is visible: dist = sqrt((px - gx)^2 + (py - gy)^2) in float64 without FMA contraction.
 * counts3 (device, uint64): [0] visible, [1] dist < thr[t], [2] dist < 3.0.  H W >= 2^24 is refused (the reference's
 * float32 sum stops being the pixel count there).  Integer atomics only: two calls give the same bits.  The host folds
 * the counts into acc_seg / acc_3px (dino_tracker_amd/tapvid.py). */
int dtk_badja_counts(const float* pred_tracks, const double* gt_tracks, const uint8_t* gt_occluded, const void* segmentations,
                     int32_t seg_is_float, float pred_scale_x, float pred_scale_y, int32_t N, int32_t T, int32_t T_seg,
                     int32_t H, int32_t W, unsigned long long* areas, unsigned long long* counts3, void* stream);

/* ---- per-video test-time training: train-mode BatchNorm2d of the Delta-DINO CNN ------------------------
 * Replaces nn.BatchNorm2d in training mode inside DeltaDINO.forward (models/networks/delta_dino.py:38,53-55; batches of
 * <= 8 frames, models/tracker.py:118-124) and its autograd backward.  x, y, dy, dx: [N][C][HW] float32 (NCHW).
 * forward:  y = gamma (x - mean_c) rstd_c + beta over the batch statistics of channel c (biased variance, eps inside the
 *   root), followed by ReLU when relu != 0 (the nn.ReLU that follows the first three layers, delta_dino.py:41-42);
 *   save_mean / save_rstd [C] for the backward; running_mean / running_var [C] (nullable) are updated in place with
 *   `momentum` and the UNBIASED batch variance, as torch does.  Statistics by pairwise (Chan) merging of exact small-group
 *   moments -- no E[x^2] - E[x]^2.
 * pre_bias [C] (nullable): the bias of the convolution in front of the layer (delta_dino.py:29-31), NOT added to x by the
 *   caller: a per-channel constant only shifts the batch mean, so it enters running_mean and nothing else -- the layer
 *   never makes the (n, C, H, W) pass that adds it.
 * backward: dx, dgamma [C], dbeta [C] from dy (the gradient w.r.t. the ReLU'd output when relu != 0); dpre_bias [C]
 *   (nullable) = sum of dx = the gradient of pre_bias: zero in exact arithmetic, the float32 rounding residue here.
 * workspace: dtk_batchnorm_workspace_bytes(C) bytes of device memory. */
size_t dtk_batchnorm_workspace_bytes(int32_t C);
int dtk_batchnorm_train_forward(const float* x, const float* gamma, const float* beta, const float* pre_bias,
                                float* running_mean, float* running_var, float momentum, float eps, int32_t relu, float* y,
                                float* save_mean, float* save_rstd, int32_t N, int32_t C, int32_t HW, void* workspace,
                                size_t workspace_bytes, void* stream);
int dtk_batchnorm_train_backward(const float* x, const float* dy, const float* gamma, const float* beta,
                                 const float* save_mean, const float* save_rstd, int32_t relu, float* dx, float* dgamma,
                                 float* dbeta, float* dpre_bias, int32_t N, int32_t C, int32_t HW, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* BlurPool of the Delta-DINO CNN (antialiased_cnns.BlurPool(channels, stride=2): filt_size 4, reflect padding, depthwise
 * outer([1,3,3,1]) / 64; models/networks/delta_dino.py:43-44) and its adjoint.  x / dx: [planes][H][W], y / dy:
 * [planes][(H-1)/2+1][(W-1)/2+1], planes = N * C; H, W >= 4. */
int dtk_blurpool_forward(const float* x, float* y, int64_t planes, int32_t H, int32_t W, void* stream);
int dtk_blurpool_backward(const float* dy, float* dx, int64_t planes, int32_t H, int32_t W, void* stream);

/* ---- N1: the convolutions of the training step as fp32-grade matrix products on the fp16 matrix cores ---------------------
 * (models/networks/delta_dino.py:29-31 under autograd; dino_tracker.py:392-448).
 * dtk_gemm_nt_f32:  C[b][m][n] (+)= sum_k A[b][m][k] * B[b][n][k]     (both operands with the reduction index contiguous)
 *   fp32 in, fp32 out; every operand is split x = hi + lo (fp16) while it is staged and a product is hi.hi + hi.lo + lo.hi
 *   with fp32 accumulation (2^-22 relative per operand).  scale_a / scale_b: DEVICE scalars (powers of two, NULL = 1) applied
 *   before the split and divided out in the epilogue, so that small operands (gradients) keep normal fp16 halves.
 *   batch b: operands b * stride_a / stride_b (0 = shared), output b * stride_c.  split_k > 1 cuts the reduction into chunks
 *   whose partial sums are ATOMICALLY added to C; accumulate: 0 overwrite, 1 C += (single writer), 2 atomic add (several
 *   batches writing the same C: stride_c = 0).  With split_k > 1 or accumulate 2 the caller zeroes / owns C's prior content.
 * dtk_im2col: unfolded operand of a stride-1 'same' convolution (2 pad == dil (k - 1)), reflect or zero padding:
 *   layout 0: cols[f][l][Kp]  (l = y W + x, k = (c ksize + ky) ksize + kx contiguous, zero-filled to Kp)
 *   layout 1: cols[f][Kp][Lp] (pixels contiguous, zero-filled to Lp)
 * dtk_col2im: adjoint of layout 1 with Lp = H W (incl. the adjoint of the reflect padding): dcols[f][Kp][H W] -> dx[f][C][H][W]
 * dtk_transpose_f32: dst[b][c][r] = src[b][r][c]. */
int dtk_gemm_nt_f32(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb,
                    int64_t ldc, int32_t batch, int64_t stride_a, int64_t stride_b, int64_t stride_c, int32_t split_k,
                    int32_t accumulate, const float* scale_a, const float* scale_b, void* stream);
/* the same with an optional batch -> operand map: batch b reads B operand number index_b[b] and writes (accumulate 2: adds to)
 * output number index_c[b]; either may be NULL (identity). */
int dtk_gemm_nt_f32_indexed(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb,
                            int64_t ldc, int32_t batch, int64_t stride_a, int64_t stride_b, int64_t stride_c, int32_t split_k,
                            int32_t accumulate, const float* scale_a, const float* scale_b, const int32_t* index_b,
                            const int32_t* index_c, void* stream);
int dtk_im2col(const float* x, float* cols, int32_t n, int32_t C, int32_t H, int32_t W, int32_t ksize, int32_t pad, int32_t dil,
               int32_t reflect, int32_t layout, int32_t Kp, int64_t Lp, void* stream);
int dtk_col2im(const float* dcols, float* dx, int32_t n, int32_t C, int32_t H, int32_t W, int32_t ksize, int32_t pad, int32_t dil,
               int32_t reflect, int32_t Kp, void* stream);
int dtk_transpose_f32(const float* src, float* dst, int64_t rows, int64_t cols, int32_t batch, void* stream);

/* CNN -> ViT grid alignment of the training step (models/utils.py:7-45), forward and backward, as a separable two-tap
 * resampling given by per-axis tables: destination index i reads source cells lo[i] and min(lo[i] + 1, n - 1) with weights
 * 1 - whi[i] and whi[i].  src / dsrc [planes][hs][ws], dst / ddst [planes][hd][wd].  Backward tables per axis: int32
 * ranges[4][n_src] = start, end of the destination indices whose LO is a, then start, end of those whose HI is a. */
int dtk_resample2d_forward(const float* src, float* dst, int64_t planes, int32_t hs, int32_t ws, int32_t hd, int32_t wd,
                           const int32_t* ylo, const float* ywhi, const int32_t* xlo, const float* xwhi, void* stream);
int dtk_resample2d_backward(const float* ddst, float* dsrc, int64_t planes, int32_t hs, int32_t ws, int32_t hd, int32_t wd,
                            const int32_t* yranges, const float* ywhi, const int32_t* xranges, const float* xwhi, void* stream);

/* Tracker.sample_embeddings of the training step (models/tracker.py:96-111 -> utils.py:65-109 for an exact frame index): pts [B][3] =
 * (x, y in [-1, 1] token-grid coordinates, frame index into the batch), feat the token-major batch embeddings [n][h w][C] ->
 * out [B][C], bilinear over the four surrounding cells, align_corners, border clamp.  The backward ACCUMULATES g [B][C] into dfeat
 * [n][h w][C] (atomic adds: several points share cells); the points carry no gradient (the reference detaches them, utils.py:91). */
int dtk_sample_bilinear_forward(const float* feat, const float* pts, float* out, int32_t B, int32_t n, int32_t h, int32_t w, int32_t C,
                                void* stream);
int dtk_sample_bilinear_backward(const float* g, const float* pts, float* dfeat, int32_t B, int32_t n, int32_t h, int32_t w, int32_t C,
                                 void* stream);

/* Operand scale of a gradient tensor for the fp16 split of the training convolutions: out[0] = 2^e with max |x| * 2^e in [2^9, 2^10]
 * (max |x| clamped below at 1e-30; a NaN in x gives NaN).  x: n floats on the device; scratch: 4 bytes on the device.  Three small
 * launches, no memset -- safe inside a captured graph (a library reduction is not, on this stack: csrc/common.h, dtk_zero_async). */
int dtk_pow2_scale(const float* x, int64_t n, float* out, void* scratch, void* stream);

/* ---- N1: the optimiser step of test-time training (dino_tracker.py:110-115: torch.optim.Adam over two parameter groups, default
 * betas / eps, no weight decay, no amsgrad; optimization/schedulers.py:4-8 scales the groups' learning rates) ---------------------
 * ONE launch updates every parameter tensor of the step: the tensors travel BY VALUE in the argument block (their gradients are
 * new allocations every iteration, so a device-side table would need a copy per step).  torch.optim.Adam's arithmetic:
 *   m <- m + (1 - beta1) (g - m);  v <- beta2 v + (1 - beta2) g g;
 *   p <- p - (lr[group] / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps),   step = the tensor's own count. */
#define DTK_ADAM_MAX_TENSORS 32
#define DTK_ADAM_MAX_GROUPS 4
typedef struct dtk_adam_args {
    float* param[DTK_ADAM_MAX_TENSORS];            /* device, fp32, updated in place */
    const float* grad[DTK_ADAM_MAX_TENSORS];       /* device, fp32 */
    float* exp_avg[DTK_ADAM_MAX_TENSORS];          /* device, fp32, updated in place (m) */
    float* exp_avg_sq[DTK_ADAM_MAX_TENSORS];       /* device, fp32, updated in place (v) */
    int64_t numel[DTK_ADAM_MAX_TENSORS];
    int32_t group[DTK_ADAM_MAX_TENSORS];           /* index into lr[] */
    int32_t step[DTK_ADAM_MAX_TENSORS];            /* per tensor: 1-based step count AFTER this update (its bias corrections; a
                                                    * parameter that had no gradient in some iteration lags behind the others) */
    int32_t n_tensors;
    double lr[DTK_ADAM_MAX_GROUPS];                /* doubles, as torch keeps them: its scalar coefficients (1 - beta2 = 0.001, lr / (1 -
                                                    * beta1^step) ...) are formed in double and rounded to fp32 ONCE; 1.f - 0.999f is 4.7e-5 off */
    double beta1, beta2, eps;
} dtk_adam_args;
int dtk_adam_step(const dtk_adam_args* a, void* stream);
/* The same update for a CAPTURED iteration (hipGraph): pointers and sizes are baked into the launch, the two per-tensor scalars --
 * step size lr[group] / (1 - beta1^step) and 1 / sqrt(1 - beta2^step) -- are read from device memory that the host refreshes before
 * every replay.  dtk_adam_scalars forms them on the host exactly as dtk_adam_step does (out_host: 2 * DTK_ADAM_MAX_TENSORS floats,
 * step sizes first; it reads n_tensors, betas, eps, group[], step[] and lr[] only -- the tensor pointers may be null);
 * dtk_adam_step_dev launches with `scalars_dev` in that layout. */
int dtk_adam_scalars(const dtk_adam_args* a, float* out_host);
int dtk_adam_step_dev(const dtk_adam_args* a, const float* scalars_dev, void* stream);

/* ---- PCA foreground masks (preprocessing/create_fg_mask.py:11-43) on a token-major fp32 volume x [N][C], C = 384, 768 or 1024 ----
 * With `normalize` every row is x^_n = x_n / max(||x_n||, 1e-12) (F.normalize), otherwise x^_n = x_n.
 *
 * dtk_pca_moments: mean[C] = (1 / N) sum_n x^_n and cov[C][C] = sum_n (x^_n - mean)(x^_n - mean)^T (NOT divided by N), in two
 * passes (mean first, then the centred Gram).  The Gram runs on the matrix cores on hi + lo fp16 planes of the centred values
 * (three products, the lo.lo one dropped: 2^-21 relative to |Xc|^T |Xc| plus the fp32 accumulation); un-normalised input must
 * stay inside the fp16 range after centring.  The tokens are split into chunks of `chunk_rows` (rounded up to a multiple of 32;
 * 0 = the library's choice) whose partial sums are reduced in index order without atomics: two calls give the same bits, and
 * cov is exactly symmetric.  Workspace: dtk_pca_moments_workspace_bytes(N, C, chunk_rows), 0 for arguments the call refuses.
 *
 * dtk_pca_project: colors[N][q] = x^_n . V[j] for V [q][C] (fp32, q <= 8; rows not centred, as the reference projects them) and
 * minmax[16]: minmax[j] = min_n colors[n][j], minmax[8 + j] = the maximum (j < q; the rest +-inf).
 *
 * dtk_fg_mask: tmp = (colors[n][comp] - min) / (max - min), 1 - tmp when `flip`; token n = (t, y, x) of the [T][h][w] grid is
 * foreground iff tmp < thr (max == min: never).  token_mask [T][h][w] and mask [T][H][W] are 0 / 255; mask is the nearest
 * upsampling of F.interpolate: destination (y, x) reads token (floor(y h / H), floor(x w / W)). */
size_t dtk_pca_moments_workspace_bytes(int64_t N, int32_t C, int64_t chunk_rows);
int dtk_pca_moments(const float* x, int64_t N, int32_t C, int32_t normalize, int64_t chunk_rows, float* mean, float* cov,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t dtk_pca_project_workspace_bytes(int64_t N);
int dtk_pca_project(const float* x, int64_t N, int32_t C, int32_t normalize, const float* V, int32_t q, float* colors,
                    float* minmax, void* workspace, size_t workspace_bytes, void* stream);
int dtk_fg_mask(const float* colors, int32_t q, int32_t comp, const float* minmax, float thr, int32_t flip, int32_t T, int32_t h,
                int32_t w, int32_t H, int32_t W, uint8_t* mask, uint8_t* token_mask, void* stream);

/* ---- Trajectories chained from optical flow (preprocessing/extract_trajectories.py:75-93, :143-158, :203-266: everything behind
 * the RAFT network) ----------------------------------------------------------------------------------------------------------------
 * Flows are fp32 pixel displacements; fflow[i] maps frame i -> i + 1 and bflow[i] frame i + 1 -> i (the reference's flows[0] and
 * flows[1]).  dtk_flow_pack turns n planar fields [n][2][h][w] into the PACKED form [n][h][w][2] every other entry reads.
 *
 * The arithmetic is the specification.  Positions are fp32 and every step is one IEEE-754 operation, never contracted, with
 * correctly rounded division and square root.  A bilinear read at (x, y) is grid_sample(align_corners=True) written out:
 *   gx = 2 x / (w - 1) - 1;  ix = ((gx + 1) / 2) (w - 1)  (y alike);  x0 = floor(ix), x1 = x0 + 1;
 *   weights (x1 - ix)(y1 - iy), (ix - x0)(y1 - iy), (x1 - ix)(iy - y0), (ix - x0)(iy - y0) for the corners (x0, y0), (x1, y0),
 *   (x0, y1), (x1, y1), the four products summed in that order from zero; a corner outside the image contributes zero.
 * "Border padding" clamps ix, iy to the image before the floor.  A distance is sqrt(dx dx + dy dy).  round() is half to even.
 *
 * dtk_flow_cycle_masks: consistent [T][h][w] (0 / 1).  consistent[0] = 0; for pixel g of frame i + 1, c = g + bflow[i](g),
 *   c' = c + bilinear(fflow[i], c): consistent[i + 1](g) = |g - c'| < threshold AND g = round(p + fflow[i](p)) for some pixel p.
 *
 * dtk_flow_traj_start, for the starting frame s (call s = 0, 1, ... in order on one stream; `visited` [T][h][w] starts zeroed):
 *   a pixel is live when consistent[s] is 0 there or visited[s] is 0 there; the live pixels, in raster order, walk
 *     x' = x + bilinear(fflow[s + k], x);  err = |x - (x' + bilinear(bflow[s + k], x'))|      k = 0 .. T - 2 - s
 *   and stay live while err < threshold and x' lies in [0, w - 1] x [0, h - 1]; the run ends at the first dead step.  With
 *   use_direct (direct_fwd / direct_back: packed [T - 1 - s][h][w][2], the flows s -> s + k + 1 and back) additionally
 *     d = start + direct_fwd[k](start);  dmask = |start - (d + bilinear_border(direct_back[k], d))| < threshold and d inside;
 *     the point stays live only while |x' - d| dmask < direct_threshold.
 *   *n_rows (device) receives the number of runs of at least min_trajectory_length frames.  No host synchronisation.
 * dtk_flow_traj_emit, with the same workspace and n_rows read back by the caller: rows [n_rows][T][2], the kept runs in raster
 *   order, NaN outside frames s .. s + length - 1; every point of a kept run sets visited[frame][round(y)][round(x)].
 * The blocks of s = 0, 1, ... concatenated are the reference's rows in the reference's order.
 * Workspace: dtk_flow_traj_workspace_bytes(T, h, w) (a [T][h w] slab of points and the compaction lists), 0 for sizes the calls
 * refuse (T < 2, h or w < 2). */
int dtk_flow_pack(const float* flow, float* packed, int32_t n, int32_t h, int32_t w, void* stream);
int dtk_flow_cycle_masks(const float* fflow_packed, const float* bflow_packed, int32_t T, int32_t h, int32_t w, float threshold,
                         uint8_t* consistent, void* stream);
size_t dtk_flow_traj_workspace_bytes(int32_t T, int32_t h, int32_t w);
int dtk_flow_traj_start(const float* fflow_packed, const float* bflow_packed, const uint8_t* consistent, const uint8_t* visited,
                        int32_t T, int32_t h, int32_t w, int32_t s, float threshold, int32_t min_trajectory_length,
                        const float* direct_fwd, const float* direct_back, int32_t use_direct, float direct_threshold,
                        int32_t* n_rows, void* workspace, size_t workspace_bytes, void* stream);
int dtk_flow_traj_emit(int32_t T, int32_t h, int32_t w, int32_t s, int32_t min_trajectory_length, int32_t n_rows, float* rows,
                       uint8_t* visited, const void* workspace, size_t workspace_bytes, void* stream);

/* ---- Track videos: dotted tracks and rainbow trails (visualization/viz_utils_tapir.py plot_tracks_v2 / plot_tracks_tails) as a
 * tiled, ordered alpha-blending rasteriser.  The picture is DEFINED in docs/RENDER.md (pixel centres, analytic one-pixel coverage
 * ramps, c <- c (1 - a cov) + colour a cov in fp32, draw order = the reference's); it is not matplotlib's Agg output. -----------
 * A primitive RECORD is DTK_RENDER_RECORD_WORDS = 12 32-bit words:
 *   [0] kind (int32: DTK_RENDER_SEGMENT / _DISC / _DIAMOND / _RING)   [1..4] x0 y0 x1 y1 (markers: both ends the centre)
 *   [5] size: half-width (segment), radius (disc, ring), L1 radius rho (diamond)  [6..8] r g b in [0, 1]      [9] a
 *   [10] 1 / |p1 - p0|^2 (0 for a zero-length segment and for markers; RING: the half stroke width hw)
 *   [11] frame in the group (int32)
 * Records are stored in draw order: frame by frame, and within a frame in the order the reference draws.
 *
 * dtk_render_prims writes the records of frames f0 .. f0 + F - 1 of a video of T frames with N points.  points [N][T][2] fp32,
 *   occluded [N][T] uint8 (0 / 1), colors [N][3] fp32.  mode DTK_RENDER_DOTTED: N markers per frame, a = 1 - occluded[n][i].
 *   mode DTK_RENDER_TAILS: maps [T][T][9] fp32 with maps[i][j] = inv(H_i) H_j (row-major 3 x 3, formed by the caller in float64;
 *   only j < i is read); frame i has N (i + 1) records: the markers, then for j = i - 1 .. 0 the N segments P(n, j) -> P(n, j + 1)
 *   with the reference's out-of-frame rule, clamping and fade (docs/RENDER.md).  A record with a = 0 bins nowhere.
 *   dtk_render_prim_count(mode, N, f0, F) is the number of records of the group.
 * dtk_render_pred_gt_prims (visualization/visualize_pred_vs_gt.py:13-38): pred_xy / gt_xy [N][T][2] int32 (already truncated
 *   by the caller), pred_occluded / gt_occluded [N][T] uint8, colors [N][3] fp32 -> exactly 2 records per (frame, point), frame
 *   by frame, ascending n: both visible: red (1, 0, 0) segment pred -> gt of half width thickness / 2, disc of `radius` in the
 *   point's colour; gt occluded only: the two diagonals (x -+ cross_size, y -+ cross_size) of half width thickness / 2 in the
 *   point's colour; pred occluded only: red segment of half width (thickness / 2 as integers) / 2, ring of `radius` with hw = 1;
 *   both occluded: two all-zero records (a = 0).  Every drawn record has a = 1.
 * dtk_render_tile_counts: counts[p] = number of DTK_RENDER_TILE x DTK_RENDER_TILE tiles the bounding box of record p meets: the
 *   extent grown by size + 0.5 (diamond: size + sqrt(1/2); ring: size + hw + 0.5), clipped to the W x H frame; 0 when a <= 0, a coordinate is not finite or the record's frame is not in 0 .. F - 1.
 * dtk_render_tile_keys: offsets[p] = exclusive prefix sum of counts (int64); writes one key per (tile, record):
 *   key = ((frame * tiles_y + ty) * tiles_x + tx) << 32 | p.  Keys are unique, so their sorted order does not depend on which
 *   thread wrote which; ascending order inside one (frame, tile) is draw order.
 * dtk_render_blend: sorted keys [K], tile_start [F tiles_y tiles_x + 1] (tile_start[t] = first key of tile t, = searchsorted of
 *   t << 32).  One workgroup of 256 threads per tile, one pixel per thread; the tile's records pass through LDS in chunks of
 *   DTK_RENDER_CHUNK.  frames_in [F][H][W][3] uint8 -> out_u8 [F][H][W][3] uint8 = floor(255 c + 0.5), and out_f32 (same shape,
 *   fp32 c) when not null.  Only plain vector stores; no atomics anywhere, so two calls give the same bits.
 * dtk_render_group_bytes: device bytes of one frame group's buffers (records, counts, offsets, keys and their sort, tile starts,
 *   input and output frames) for `prims` records and `keys` keys; the caller sizes its frame groups with it.  0 for bad sizes. */
#define DTK_RENDER_SEGMENT 0
#define DTK_RENDER_DISC 1
#define DTK_RENDER_DIAMOND 2
#define DTK_RENDER_RING 3 /* stroked circle: coverage clamp(0.5 + hw - |d - r|, 0, 1) */
#define DTK_RENDER_DOTTED 0
#define DTK_RENDER_TAILS 1
#define DTK_RENDER_RECORD_WORDS 12
#define DTK_RENDER_TILE 16
#define DTK_RENDER_CHUNK 256
int64_t dtk_render_prim_count(int32_t mode, int32_t N, int32_t f0, int32_t F);
size_t dtk_render_group_bytes(int64_t prims, int64_t keys, int32_t F, int32_t H, int32_t W);
int dtk_render_prims(const float* points, const uint8_t* occluded, const float* maps, const float* colors, int32_t N, int32_t T,
                     int32_t f0, int32_t F, int32_t H, int32_t W, int32_t mode, int32_t marker_kind, float marker_size,
                     float half_width, int32_t trail_fade, float* records, void* stream);
int dtk_render_pred_gt_prims(const int32_t* pred_xy, const int32_t* gt_xy, const uint8_t* pred_occluded,
                             const uint8_t* gt_occluded, const float* colors, int32_t N, int32_t T, int32_t f0, int32_t F,
                             int32_t thickness, int32_t radius, int32_t cross_size, float* records, void* stream);
int dtk_render_tile_counts(const float* records, int64_t P, int32_t F, int32_t H, int32_t W, int32_t* counts, void* stream);
int dtk_render_tile_keys(const float* records, const int64_t* offsets, int64_t P, int32_t F, int32_t H, int32_t W, int64_t K,
                         int64_t* keys, void* stream);
int dtk_render_blend(const uint8_t* frames_in, const float* records, int64_t P, const int64_t* sorted_keys, int64_t K,
                     const int64_t* tile_start, int32_t F, int32_t H, int32_t W, uint8_t* out_u8, float* out_f32, void* stream);

/* ---- Video ingest: Pillow's 8-bit separable resampler (Image.resize on uint8, src/libImaging/Resample.c) on the device ---------
 * dtk_resize_u8 resamples N frames  in [N][H][W][C] uint8 (interleaved, C = 1 or 3)  to  h x w.  out_form:
 *   DTK_RESIZE_OUT_U8_HWC  : out [N][h][w][C] uint8
 *   DTK_RESIZE_OUT_F32_CHW : out [N][C][h][w] fp32 = u8_to_f32[value]  (the caller's 256-entry table: ToTensor's u8 / 255 as the
 *                            host rounds it, so the bits do not depend on the device's division)
 * The filter lives in the caller's tables (device pointers), per axis:  k [out][ksize] int32 weights in 22-bit fixed point and
 *   b [out][2] int32 (first input index, count <= ksize); rows of k beyond `count` are not read.  The kernels never evaluate a
 *   filter.  Arithmetic, per pass:  acc = 2^21 + sum_j in[first + j] * k[j]  in int32,  out = clamp(acc >> 22, 0, 255)  (arithmetic
 *   shift); horizontal pass first, vertical pass on its uint8 result.  The products are formed by 24-bit multiplies: |k| < 2^23,
 *   and the caller guarantees 255 * sum|k| + 2^21 < 2^31 per row.  A pass whose sizes are equal (W == w, H == h) is skipped and
 *   its tables are not read (they may be null).  Bounds are clamped to the frame before use: a bad table gives wrong pixels, never
 *   an access outside the buffers.
 * Two forms.  FUSED: one workgroup per DTK_RESIZE_TILE_H x DTK_RESIZE_TILE_W output tile runs the horizontal pass for the input
 *   rows the tile needs into LDS (uint8), the vertical pass from LDS, and writes the output in its final form; the input is read
 *   once (plus the rows neighbouring tiles share), nothing else touches memory.  It is taken when the rows of one tile,
 *   min(H, (TILE_H - 1) * H / h + ksize_y + 1) of them (TILE_H when the vertical pass is skipped), fit in 64 KiB of LDS at
 *   TILE_W * C bytes each -- the caller's vertical bounds must stay inside that span, as those of any resampling filter of
 *   support (ksize_y - 1) / 2 do.  GENERAL: one launch per pass with the uint8 intermediate [N][H][w][C] in `workspace`
 *   (dtk_resize_workspace_bytes; 0 when the fused form is taken or a pass is skipped).  DTK_RESIZE_FORCE_GENERAL in `options`
 *   selects the general form regardless. */
#define DTK_RESIZE_OUT_U8_HWC 0
#define DTK_RESIZE_OUT_F32_CHW 1
#define DTK_RESIZE_FORCE_GENERAL 1
#define DTK_RESIZE_TILE_H 32
#define DTK_RESIZE_TILE_W 64
size_t dtk_resize_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t h, int32_t w, int32_t ksize_y,
                                  int32_t options);
int dtk_resize_u8(const uint8_t* in, int32_t N, int32_t H, int32_t W, int32_t C, int32_t h, int32_t w, const int32_t* kx,
                  const int32_t* bx, int32_t ksize_x, const int32_t* ky, const int32_t* by, int32_t ksize_y,
                  const float* u8_to_f32, int32_t out_form, int32_t options, void* out, void* workspace, size_t workspace_bytes,
                  void* stream);

/* ---- RAFT-large optical flow (torchvision.models.optical_flow.raft_large, restated from the published definition: the one step
 * of preprocessing/extract_trajectories.py the entries above did not cover) ----------------------------------------------------
 * Every activation is fp32 NHWC: [images][rows][columns][channels].  A tensor argument may be a channel SLICE of a wider tensor:
 * a pointer to the slice's first channel of pixel 0 plus the channel stride (floats from one pixel to the next).
 *
 * Operand modes (`mode`), for the convolutions and the correlation:
 *   DTK_RAFT_SPLIT  every operand x is carried as hi + lo, hi = fp16(x), lo = fp16(x - hi), and every product a b is formed as
 *                   a_hi b_hi + a_hi b_lo + a_lo b_hi on the matrix cores with fp32 accumulation.  Representation: hi + lo equals
 *                   x to max(2^-22 |x|, 2^-25) for |x| < 65504; the dropped a_lo b_lo is below 2^-22 |a b|.  Weights are packed
 *                   multiplied by the power of two `wscale` (the accumulator is multiplied by inv_wscale = 1 / wscale) so that
 *                   their lo halves stay normal numbers: for 2^-14 <= |w wscale| < 65504 the weight term is 2^-22 |w|.
 *   DTK_RAFT_FP16   the hi halves only: operands rounded to fp16 (2^-11 relative), fp32 accumulation.
 *
 * dtk_raft_conv_pack: fp32 weights [cout][cin][kh][kw] -> the planes w_hi / w_lo, dtk_raft_conv_packed_halves(cout, cin, kh, kw)
 *   fp16 values each: [cout padded to 64][kh kw][cin padded to 32] of w * wscale, zeros in the padding.
 * dtk_raft_conv: out[n][oy][ox][co] = E(inv_wscale * sum_{ky, kx, ci} in[n][oy stride - pad_h + ky][ox stride - pad_w + kx][ci]
 *   w[co][ci][ky][kx] + bias[co]), zeros outside the image, output size floor((H + 2 pad_h - kh) / stride) + 1 (W alike).  The
 *   input channels ci < in_split come from `in`, the others from `in2` (in2 = NULL: all from `in`; in_split is a multiple of 32).
 *   The epilogue E, in this order:  t = act(.) (none / max(t, 0) / sigmoid / tanh);  mul: t = t * mul;  gate: t = (1 - gate) * out_old
 *   + gate * t with out_old the value `out` held (the GRU update, in place);  res: t = t + res, then max(t, 0) when res_relu.  `res`
 *   may be `out` itself (flow += delta).  sigmoid and tanh are within 4.8e-7 absolute of the exact functions.  Only the `cout`
 *   channels of the output slice are written.  The sum runs over 32-channel chunks of one tap at a time, taps in (ky, kx) order.
 * dtk_raft_instance_norm (InstanceNorm2d, no affine, biased variance): y = (x - mean) / sqrt(var + eps) per image and channel;
 *   relu: y = max(y, 0);  res != NULL: y = max(res + y, 0).  out may be x.  Two launches, no atomics: the statistics are partial
 *   (count, mean, M2) per pixel chunk, combined in chunk order in float64 by every block alike.  C <= 256.
 * dtk_raft_corr_pyramid: f1, f2 [N][h w][C] (C a multiple of 32) -> pyramid: level 0 [N][h w][h][w] with
 *   corr[n][i][j] = <f1[n][i], f2[n][j]> / sqrt(C) in the operand mode, then levels 1 .. 3 [N][h w][h_l][w_l], h_l = floor(h_{l-1} /
 *   2): ((a + b) + (c + d)) * 0.25 of the 2 x 2 block (top-left, top-right, bottom-left, bottom-right), the odd last row / column
 *   dropped.  The levels follow each other in memory; dtk_raft_pyramid_floats(N, h, w) floats in all.  h, w >= 16.
 * dtk_raft_lookup: flow slices [N h w][2] (x, y) -> out slices [N h w][324].  For level l: x = (column + flow_x) / 2^l,
 *   y = (row + flow_y) / 2^l;  x0 = floor(x), fx = x - x0 (y alike).  Channel 81 l + 9 a + b reads level l's map of the cell at
 *   (x + a - 4, y + b - 4) -- the SLOW window index moves x, upstream's order --: corners (X, Y), (X + 1, Y), (X, Y + 1),
 *   (X + 1, Y + 1), X = x0 + a - 4, Y = y0 + b - 4, weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy, the four products
 *   summed in that order from zero; a corner outside the map contributes zero.
 * dtk_raft_upsample: mask [N h w][576] (channel 64 k + 8 dy + dx), flow slices -> out [N][2][8 h][8 w]:
 *   out[n][c][8 y + dy][8 x + dx] = sum_k softmax_k(mask) * 8 flow_c(y + k / 3 - 1, x + k % 3 - 1), zero flow outside the map;
 *   softmax as exp(mask_k - max) / sum, exp within 4.8e-7 relative, sums over k = 0 .. 8 in order.
 *
 * dtk_raft_forward: image1, image2 [N][3][H][W] fp32 in [-1, 1] -> flow_out [N][2][H][W], the LAST of num_flow_updates
 *   predictions.  model->conv[k] are the network's convolutions in the order of the DTK_RAFT_* indices below (an encoder's 16:
 *   stem; layer1 block 1 conv 1, 2; block 2 conv 1, 2; layer2 block 1 conv 1, 2, downsample; block 2 conv 1, 2; layer3 alike;
 *   output).  The feature encoder normalises with dtk_raft_instance_norm (eps 1e-5); the context encoder's BatchNorms are folded
 *   into its convolutions by the caller, and its output convolution is given as two (hidden half: tanh; context half: ReLU).
 *   The mask predictor's 0.25 is folded into its last convolution by the caller.  flow is updated as flow += delta.
 *   Refused with DTK_E_INVALID before anything is written: H or W not divisible by 8, a feature map below 16 x 16, host or null
 *   pointers; a short workspace with DTK_E_WORKSPACE.  dtk_raft_workspace_bytes(N, H, W): the encoder activations (three
 *   buffers of 2 N (H / 2)(W / 2) 64 floats), the update block's buffers and the pyramid (N (h w) (h w + ...) floats: ~220 MB per
 *   pair at 480 x 856 -- the caller bounds its batch by this); 0 for sizes the call refuses. */
#define DTK_RAFT_SPLIT 0
#define DTK_RAFT_FP16 1
#define DTK_RAFT_ACT_NONE 0
#define DTK_RAFT_ACT_RELU 1
#define DTK_RAFT_ACT_SIGMOID 2
#define DTK_RAFT_ACT_TANH 3
#define DTK_RAFT_FEATURE 0          /* .. 15 */
#define DTK_RAFT_CONTEXT 16         /* .. 30, then the two halves of the output convolution */
#define DTK_RAFT_CONTEXT_HIDDEN 31
#define DTK_RAFT_CONTEXT_CONTEXT 32
#define DTK_RAFT_MOTION 33          /* convcorr1, convcorr2, convflow1, convflow2, conv */
#define DTK_RAFT_GRU 38             /* convgru1 z, r, q; convgru2 z, r, q */
#define DTK_RAFT_FLOW_HEAD 44       /* conv1, conv2 */
#define DTK_RAFT_MASK 46            /* the 3 x 3 convolution, the 1 x 1 convolution (x 0.25 folded) */
#define DTK_RAFT_NUM_CONVS 48
typedef struct dtk_raft_conv_desc {
    const void* w_hi;   /* dtk_raft_conv_pack's planes; w_lo may be NULL for DTK_RAFT_FP16 */
    const void* w_lo;
    const float* bias;  /* [cout] */
    int32_t cin, cout, kh, kw, stride, pad_h, pad_w;
    float inv_wscale;
} dtk_raft_conv_desc;
typedef struct dtk_raft_conv_args {
    dtk_raft_conv_desc conv;
    int32_t N, H, W, mode, act, res_relu, in_split, reserved;
    const float* in;
    const float* in2;
    float* out;
    const float* res;
    const float* mul;
    const float* gate;
    int64_t in_stride, in2_stride, out_stride, res_stride, mul_stride, gate_stride;
} dtk_raft_conv_args;
typedef struct dtk_raft_model {
    dtk_raft_conv_desc conv[DTK_RAFT_NUM_CONVS];
} dtk_raft_model;
size_t dtk_raft_conv_packed_halves(int32_t cout, int32_t cin, int32_t kh, int32_t kw);
int dtk_raft_conv_pack(const float* w, int32_t cout, int32_t cin, int32_t kh, int32_t kw, float wscale, void* w_hi, void* w_lo,
                       void* stream);
int dtk_raft_conv(const dtk_raft_conv_args* args, void* stream);
size_t dtk_raft_instance_norm_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C);
int dtk_raft_instance_norm(const float* x, const float* res, float* out, int32_t N, int32_t H, int32_t W, int32_t C, float eps,
                           int32_t relu, void* workspace, size_t workspace_bytes, void* stream);
size_t dtk_raft_pyramid_floats(int32_t N, int32_t h, int32_t w);
int dtk_raft_corr_pyramid(const float* f1, const float* f2, int32_t N, int32_t h, int32_t w, int32_t C, int32_t mode, float* pyramid,
                          void* stream);
int dtk_raft_lookup(const float* pyramid, const float* flow, int64_t flow_stride, int32_t N, int32_t h, int32_t w, float* out,
                    int64_t out_stride, void* stream);
int dtk_raft_upsample(const float* flow, int64_t flow_stride, const float* mask, int32_t N, int32_t h, int32_t w, float* out,
                      void* stream);
size_t dtk_raft_workspace_bytes(int32_t N, int32_t H, int32_t W);
int dtk_raft_forward(const dtk_raft_model* model, const float* image1, const float* image2, int32_t N, int32_t H, int32_t W,
                     int32_t num_flow_updates, int32_t mode, float* flow_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Video output: baseline JPEG (SOF0, 8 bit, Y 2 x 2 + Cb + Cr: 4:2:0, one interleaved scan, restart interval
 * DTK_JPEG_RESTART MCUs, the typical Huffman tables of Annex K) of rendered frames, for Motion-JPEG AVIs and frame folders.  The
 * arithmetic is DEFINED in docs/JPEG.md and is integer throughout; the kernels never evaluate a cosine or a quality setting. -----
 * frames [F][H][W][3] uint8 (interleaved RGB).  An MCU is 16 x 16 pixels, mw = ceil(W / 16), mh = ceil(H / 16), MCUs in raster order,
 * blocks of an MCU in the order Y00 Y01 Y10 Y11 Cb Cr.  qtables: uint8 [2][64], the luma and the chroma quantisation table in ZIGZAG
 * order, values 1 .. 255 -- the 64 bytes a DQT segment stores; a zero entry is the caller's error (a division by zero on the device
 * yields garbage coefficients, nothing else).
 *
 * dtk_jpeg_coefficients: the transform stage alone.  coef_out int16 [F][mh mw][6][64], zigzag order, operation by operation:
 *   colour:   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,  Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16,
 *             Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16  (arithmetic shifts).
 *   edges:    Y(y, x) = Y(min(y, H - 1), min(x, W - 1)).  Chroma row r, column c averages the colour planes at rows 2 r', 2 r' + 1
 *             (clamped to H - 1) with r' = min(r, ceil(H / 2) - 1) and columns 2 c, 2 c + 1 (clamped to W - 1):
 *             (a + b + c + d + bias) >> 2, bias = 1 for even c, 2 for odd c.  So the last DOWNSAMPLED row repeats downwards.
 *   dummy:    a Y block whose block column is >= ceil(W / 8) or whose block row is >= ceil(H / 8) is not transformed: its AC
 *             coefficients are 0 and its DC is the quantised DC of the previous block of its MCU.
 *   DCT:      samples - 128, the separable 13-bit fixed-point transform of docs/JPEG.md section 3, rows first (8 x the DCT).
 *   quantise: q8 = 8 Q[k];  c >= 0: (c + q8 / 2) / q8;  c < 0: -((-c + q8 / 2) / q8), truncating divisions.
 * dtk_jpeg_encode: transform, entropy coding, assembly.  header [header_bytes] is the caller's file header SOI .. SOS (device
 *   pointer; it must declare DRI = DTK_JPEG_RESTART and the Annex K tables, docs/JPEG.md section 5) and is copied in front of
 *   every frame's scan.  out receives the F files one after the other:  header, the restart intervals with FF D0+n (n = the
 *   interval's index - 1 modulo 8) in front of all but the first, FF D9.  Within an interval: DC differences against the previous
 *   block of the component (0 at the interval's start), run/size symbols with ZRL and EOB, bits MSB first, the last byte completed
 *   with 1-bits, a 0x00 after every 0xFF data byte.  offsets int64 [F + 1]: file f is out[offsets[f] .. offsets[f + 1]);
 *   *needed (int64) = offsets[F].  offsets and *needed are always written.  If *needed > out_capacity NOTHING is written to out and
 *   the call still returns 0: the caller reads *needed and calls again with a buffer of that size.
 *   workspace: dtk_jpeg_workspace_bytes(F, H, W) bytes, 256-byte aligned: the coefficients (768 bytes per MCU), one slot of
 *   DTK_JPEG_INTERVAL_BYTES per restart interval (an interval's worst case: 16 MCUs x 6 blocks x (20 + 63 x 26) bits, doubled by
 *   stuffing) and the interval tables -- about 13 bytes per pixel, so the caller bounds F by it.  No host synchronisation inside.
 * Refused with DTK_E_INVALID before anything is launched: F < 1, H or W < 1, H or W > 65535, null pointers, header_bytes < 1;
 *   dtk_jpeg_workspace_bytes returns 0 for such sizes. */
#define DTK_JPEG_RESTART 16
#define DTK_JPEG_INTERVAL_BYTES 39808 /* >= 2 * 16 * 6 * 1658 / 8 = 39792, rounded to 64 */
size_t dtk_jpeg_workspace_bytes(int32_t F, int32_t H, int32_t W);
int dtk_jpeg_coefficients(const uint8_t* frames, int32_t F, int32_t H, int32_t W, const uint8_t* qtables, int16_t* coef_out,
                          void* stream);
int dtk_jpeg_encode(const uint8_t* frames, int32_t F, int32_t H, int32_t W, const uint8_t* qtables, const uint8_t* header,
                    int32_t header_bytes, uint8_t* out, size_t out_capacity, int64_t* offsets, int64_t* needed, void* workspace,
                    void* stream);

/* ---- Video ingest: baseline JPEG DECODING (SOF0, 8 bit, components 1 2 3 in one interleaved scan -- sampled 4:2:0, 4:2:2 or 4:4:4,
 * the DTK_JPEG_* samplings below -- or one gray component, 8-bit quantisation tables, the file's own Huffman tables, any restart
 * interval).  The arithmetic is DEFINED in docs/JPEG_DECODE.md -- libjpeg-turbo's default path: slow-integer IDCT, "fancy" h2v2 / h2v1
 * upsampling, replication where the chroma plane is at most two samples wide -- and is integer throughout.  The header is the CALLER's
 * to parse and validate (dino_tracker_amd/video_in.py); the library sees tables and a table of segments. --------------------------
 * dtk_jpeg_decode_coefficients: the entropy stage.  stream [stream_bytes]: the files' bytes (device).  A SEGMENT is a run of
 *   entropy-coded bytes that starts byte-aligned with the DC predictors at 0 -- a restart interval without its RSTn marker, or a
 *   whole scan -- and holds whole MCUs: int64 [n_segments][DTK_JPEG_SEGMENT_FIELDS] = frame, byte offset in stream, byte length,
 *   first MCU, MCU count.  The table is passed twice: `segments` on the device (read by the kernel) and `segments_host`, the same
 *   values in host memory, which are checked BEFORE anything is launched (the call never waits for the device).  The kernel repeats
 *   the check on its own copy: an entry that does not fit sets DTK_JPEG_S_SEGMENT and decodes nothing.  Segments of one frame
 *   must not overlap in MCUs (the caller's business: overlapping ones race on coef_out, nothing else).
 *   huffman: uint8 [F][3][2][DTK_JPEG_HUFF_BYTES]: per frame and component the DC and the AC table as a DHT stores them, 16 counts
 *   and the symbols in code order, zero-filled to 272 bytes.  The caller validates them (counts sum <= 256, no over-subscribed
 *   length, DC symbols <= 11, AC sizes <= 10); the kernel is memory-safe for any content.
 *   coef_out int16 [F][mh mw][6][64]: zigzag order, blocks Y00 Y01 Y10 Y11 Cb Cr, the encoder's layout.  Only the blocks of MCUs
 *   that some segment covers are written.  status int32 [F]: zeroed, then the OR of DTK_JPEG_S_* over the frame's segments.  A
 *   segment stops decoding at its first CODE / INDEX / OVERRUN fault; its remaining blocks are written as zeros.
 * dtk_jpeg_pixels: dequantisation, inverse DCT, upsampling, colour.  qtables uint8 [F][3][64]: per frame and component, zigzag
 *   order.  out uint8 [F][H][W][3] interleaved RGB.  status (may be null): DTK_JPEG_S_RANGE is ORed in where |coef * Q| > 2047;
 *   the arithmetic is 32-bit wrap-around, so the output is defined for any coefficients.  workspace:
 *   dtk_jpeg_decode_workspace_bytes(F, H, W) bytes, 256-byte aligned: the Y, Cb, Cr planes padded to whole MCUs (384 bytes per MCU).
 * No host synchronisation inside.  Refused with DTK_E_INVALID before anything is launched: F < 1, H or W < 1 or > 65535, null
 *   pointers, stream_bytes < 1, n_segments < 1, a segments_host entry outside the frames, the stream or the MCUs;
 *   dtk_jpeg_decode_workspace_bytes returns 0 for such sizes.
 * The three entry points above are the 4:2:0 case of the *_sampled ones, which take the sampling first and differ only in what follows
 *   from it.  With B blocks per MCU (in scan order) and an MCU of MW x MH pixels:
 *     DTK_JPEG_420   components 2x2 1x1 1x1   B = 6: Y00 Y01 Y10 Y11 Cb Cr   16 x 16
 *     DTK_JPEG_422   components 2x1 1x1 1x1   B = 4: Y0 Y1 Cb Cr             16 wide x 8 high
 *     DTK_JPEG_444   components 1x1 1x1 1x1   B = 3: Y Cb Cr                 8 x 8
 *     DTK_JPEG_GRAY  one component            B = 1: Y                       8 x 8  (a single-component scan is not interleaved:
 *                                                                            one block per MCU whatever factors its SOF names)
 *   a frame has mh mw = ceil(H / MH) ceil(W / MW) MCUs; a segment's first MCU and MCU count (and a restart interval) count those.
 *   huffman: uint8 [F][C][2][DTK_JPEG_HUFF_BYTES] and qtables: uint8 [F][C][64] with C = 3 components, 1 for DTK_JPEG_GRAY.
 *   coef: int16 [F][mh mw][B][64].  out: uint8 [F][H][W][3], for DTK_JPEG_GRAY uint8 [F][H][W].  workspace:
 *   dtk_jpeg_decode_workspace_bytes_sampled(sampling, F, H, W) bytes: the planes padded to whole MCUs, 64 B bytes per MCU.
 *   Refused with DTK_E_INVALID as above, and for a sampling that is none of the four (workspace bytes: 0). */
#define DTK_JPEG_420 0
#define DTK_JPEG_422 1
#define DTK_JPEG_444 2
#define DTK_JPEG_GRAY 3
#define DTK_JPEG_SEGMENT_FIELDS 5
#define DTK_JPEG_HUFF_BYTES 272
#define DTK_JPEG_S_CODE 1     /* no Huffman code matches the next bits */
#define DTK_JPEG_S_INDEX 2    /* a run carried the coefficient index beyond 63 */
#define DTK_JPEG_S_OVERRUN 4  /* bits were read past the segment's end */
#define DTK_JPEG_S_LEFTOVER 8 /* more than 7 unread bits at the segment's end */
#define DTK_JPEG_S_RANGE 16   /* |coefficient * Q| > 2047 */
#define DTK_JPEG_S_SEGMENT 32 /* a segment entry outside the stream or the frame */
size_t dtk_jpeg_decode_workspace_bytes(int32_t F, int32_t H, int32_t W);
int dtk_jpeg_decode_coefficients(const uint8_t* stream, int64_t stream_bytes, const int64_t* segments, const int64_t* segments_host,
                                 int32_t n_segments, const uint8_t* huffman, int32_t F, int32_t H, int32_t W, int16_t* coef_out,
                                 int32_t* status, void* stream_handle);
int dtk_jpeg_pixels(const int16_t* coef, const uint8_t* qtables, int32_t F, int32_t H, int32_t W, uint8_t* out, int32_t* status,
                    void* workspace, void* stream);
size_t dtk_jpeg_decode_workspace_bytes_sampled(int32_t sampling, int32_t F, int32_t H, int32_t W);
int dtk_jpeg_decode_coefficients_sampled(int32_t sampling, const uint8_t* stream, int64_t stream_bytes, const int64_t* segments,
                                         const int64_t* segments_host, int32_t n_segments, const uint8_t* huffman, int32_t F, int32_t H,
                                         int32_t W, int16_t* coef_out, int32_t* status, void* stream_handle);
int dtk_jpeg_pixels_sampled(int32_t sampling, const int16_t* coef, const uint8_t* qtables, int32_t F, int32_t H, int32_t W, uint8_t* out,
                            int32_t* status, void* workspace, void* stream);

/* dtk_jpeg_decode_coefficients_parallel (csrc/jpeg_parallel.hip; docs/JPEG_DECODE.md section 1b): the entropy stage of
 *   dtk_jpeg_decode_coefficients_sampled with MANY lanes per segment -- one workgroup per segment, the segment's unstuffed bytes cut
 *   into sub-streams of subseq_bytes bytes whose entry states are iterated to their fixpoint.  Arguments, coefficients and status are
 *   those of dtk_jpeg_decode_coefficients_sampled, for any bytes and any tables; what follows (dtk_jpeg_pixels_sampled) is unchanged.
 *   subseq_bytes: 0 for the default (128), else a multiple of 4 in 16 .. 1024.  workspace:
 *   dtk_jpeg_decode_parallel_workspace_bytes(sampling, stream_bytes, n_segments, subseq_bytes) bytes, 256-byte aligned: the unstuffed
 *   bytes, a state and a block count per sub-stream.  A segment's place in it follows from its byte range, so here the rows of
 *   segments_host must not overlap in bytes and must rise with the row index (what a parser emits); the device copy is to hold the same
 *   values -- one that does not stays memory-safe (DTK_JPEG_S_SEGMENT where its place would leave the workspace).
 *   No host synchronisation inside.  Refused with DTK_E_INVALID before anything is launched: what
 *   dtk_jpeg_decode_coefficients_sampled refuses, a subseq_bytes outside the above, a null workspace, rows whose bytes overlap or
 *   fall; the workspace size is 0 for such arguments.  Baseline segments only: a progressive scan's refinements depend on earlier
 *   coefficients. */
size_t dtk_jpeg_decode_parallel_workspace_bytes(int32_t sampling, int64_t stream_bytes, int32_t n_segments, int32_t subseq_bytes);
int dtk_jpeg_decode_coefficients_parallel(int32_t sampling, const uint8_t* stream, int64_t stream_bytes, const int64_t* segments,
                                          const int64_t* segments_host, int32_t n_segments, const uint8_t* huffman, int32_t F, int32_t H,
                                          int32_t W, int32_t subseq_bytes, int16_t* coef_out, int32_t* status, void* workspace,
                                          void* stream_handle);

/* ---- Video ingest: PROGRESSIVE JPEG (SOF2, 8 bit, Huffman, the four samplings above; docs/JPEG_DECODE.md "Progressive files"): the
 * entropy stage alone.  It fills the coefficient layout of dtk_jpeg_decode_coefficients_sampled, so dtk_jpeg_pixels_sampled follows
 * unchanged.  The header, the legality and completeness of the scan script and the LEVELS are the caller's
 * (dino_tracker_amd/video_in.py: parse_jpeg_progressive, scan_levels, plan_jpeg_progressive). ------------------------------------
 * dtk_jpeg_decode_progressive: a SEGMENT is a restart interval of ONE scan (or the whole scan).  segments / segments_host: int64
 *   [n_segments][DTK_JPEG_PROG_FIELDS], on the device and the same values on the host, one row per segment:
 *      0 frame          1 byte offset in stream   2 byte length (<= 2^28)   3 level (0 .. 255)
 *      4 Ss   5 Se      6 Ah   7 Al               the scan's band and bit positions: Ss = Se = 0 (DC) or 1 <= Ss <= Se <= 63 (AC);
 *                                                 Al <= 13; Ah = 0 (the band's first scan) or Ah = Al + 1 (a refinement)
 *      8 component      0 .. C - 1, or -1: the DC scan of all three components interleaved (not for DTK_JPEG_GRAY, DC only)
 *      9 first unit    10 unit count (>= 1)       a unit is an MCU of the interleaved scan, else one block of the component's REAL
 *                                                 grid -- ceil(ceil(H v_c / v_max) / 8) rows of ceil(ceil(W h_c / h_max) / 8)
 *                                                 blocks, in raster order
 *     11 12 13 tables   rows of `tables`: a DC first scan names its DC table per component (11 alone for one component), an AC scan
 *                       its AC table in 11; what a scan does not use is ignored
 *   The rows are ordered by level; all rows of one level are decoded by ONE launch, one wave per row, and the launches follow each
 *   other on the stream.  Rows of one level must not write the same coefficient of the same block: the caller gives a scan a higher
 *   level than every earlier scan of the same component whose band intersects its own.  Every host row is checked against
 *   stream_bytes, F, the unit count that follows from the sampling, the component and H x W, n_tables and the level order BEFORE
 *   anything is launched (DTK_E_INVALID); the kernel repeats the check on the device copy and sets DTK_JPEG_S_SEGMENT for a row that
 *   fails it, which decodes nothing.
 *   tables uint8 [n_tables][DTK_JPEG_HUFF_BYTES]: raw tables as a DHT stores them (validated by the caller; memory-safe for any
 *   content).  coef int16 [F][mh mw][B][64] and status int32 [F] are ZEROED here first.  Status: the DTK_JPEG_S_* bits above --
 *   CODE also for a refinement symbol whose size is neither 0 nor 1, INDEX also for a run or skip beyond Se and for an end-of-band
 *   run longer than the blocks left in the segment.  A segment stops at its first CODE / INDEX / OVERRUN and writes nothing further.
 *   No host synchronisation inside. */
#define DTK_JPEG_PROG_FIELDS 14
int dtk_jpeg_decode_progressive(int32_t sampling, const uint8_t* stream, int64_t stream_bytes, const int64_t* segments,
                                const int64_t* segments_host, int32_t n_segments, const uint8_t* tables, int32_t n_tables, int32_t F,
                                int32_t H, int32_t W, int16_t* coef, int32_t* status, void* stream_handle);

/* ---- Video and mask ingest: PNG DECODING (docs/PNG_DECODE.md): zlib / DEFLATE streams, their Adler-32, the PNG row filters.  The
 * file is the CALLER's to parse (dino_tracker_amd/png_in.py: signature, IHDR, PLTE, the IDAT payloads joined into one stream per
 * frame); the library sees byte streams and raw scanlines.  Everything is exact: the format is lossless. ------------------------------
 * dtk_inflate: n_streams independent zlib (RFC 1950, wrapper = 1: two header bytes, DEFLATE data, the Adler-32 trailer) or raw
 *   DEFLATE (RFC 1951, wrapper = 0) streams: stored, fixed and dynamic blocks, any number of them, the 32 KiB window.  in [in_bytes]
 *   (device).  streams int64 [n_streams][DTK_INFLATE_STREAM_FIELDS] = byte offset in `in`, byte length (<= 2^28), byte offset in `out`,
 *   EXPECTED output bytes (<= 2^30; a PNG frame: H (1 + W bpp)).  The table is passed twice: `streams` on the device (read by the
 *   kernel) and `streams_host`, the same values in host memory, which are checked BEFORE anything is launched (the call never waits for
 *   the device).  The kernel repeats the range check on its own copy: an entry that does not fit sets DTK_INFLATE_S_STREAM and decodes
 *   nothing.  out [out_bytes] uint8.  status int32 [n_streams]: zeroed, then the stream's DTK_INFLATE_S_* bits.  A stream stops at its
 *   FIRST fault; what it had decoded stays and the rest of its output range is written as zeros, so every byte of every range is
 *   written.  With wrapper = 1 the stream must hold at least four bytes after the final block; they are compared by dtk_adler32.
 *   The kernel is memory-safe and terminates for any input bytes: reads are bounded by the stream's end, writes by its output range,
 *   and every loop iteration consumes at least one bit or produces at least one byte.
 * dtk_adler32: the Adler-32 (s1 = 1 + sum d[i], s2 = N + sum (N - i) d[i], both mod 65521, from block sums) of every stream's output
 *   range against the big-endian value in the stream's LAST four bytes; a mismatch ORs DTK_INFLATE_S_ADLER into status[s].  A stream
 *   whose status is already non-zero is skipped (its output is not what the trailer describes); status is NOT zeroed.  Same tables.
 * dtk_png_unfilter: raw [F][H][1 + W bpp] (filter byte + scanline, what the zlib stream of an 8-bit non-interlaced PNG holds), bpp = 1
 *   (grey or palette index) or 3 (RGB) -> out uint8 [F][H][W][bpp].  Filters 0 .. 4 (None, Sub, Up, Average, Paeth) as the PNG
 *   specification defines them: arithmetic mod 256 on RECONSTRUCTED bytes, Average = floor((left + up) / 2), Paeth ties in the order
 *   left, up, up-left; bytes outside the image are 0.  A filter byte > 4 ORs DTK_PNG_S_FILTER into status[f] (int32 [F], NOT zeroed:
 *   it continues dtk_inflate's) and the row is taken as filter 0.  lut (may be null; bpp = 1 only) uint8 [F][256]: out = lut[f][value]
 *   -- a palette's grey levels -- while the filters run on the untranslated bytes.  workspace:
 *   dtk_png_unfilter_workspace_bytes(F, H, W, bpp) bytes, 256-byte aligned (one packed row per frame).
 * No host synchronisation inside.  Refused with DTK_E_INVALID before anything is launched: null pointers, in_bytes, out_bytes or
 *   n_streams < 1, wrapper other than 0 / 1, a streams_host entry outside the buffers, output ranges that overlap; F < 1, H or W < 1
 *   or > 65535, bpp other than 1 / 3, lut with bpp = 3; dtk_png_unfilter_workspace_bytes returns 0 for such sizes. */
#define DTK_INFLATE_STREAM_FIELDS 4
#define DTK_INFLATE_S_HEADER 1     /* zlib header: CM != 8, window > 32 K, FCHECK fails, or FDICT set */
#define DTK_INFLATE_S_BTYPE 2      /* block type 3 */
#define DTK_INFLATE_S_STORED 4     /* a stored block's LEN != ~NLEN */
#define DTK_INFLATE_S_TABLE 8      /* HLIT > 286, HDIST > 30; a repeat code with no previous length or beyond the count; an
                                      over-subscribed code; an incomplete code other than a distance code with a single length-1 entry
                                      (or none); no end-of-block code */
#define DTK_INFLATE_S_CODE 16      /* literal/length symbol 286 / 287, distance symbol 30 / 31, or no code matches */
#define DTK_INFLATE_S_DISTANCE 32  /* a back-reference before the stream's first output byte */
#define DTK_INFLATE_S_OVERRUN 64   /* input exhausted */
#define DTK_INFLATE_S_LENGTH 128   /* output would exceed the expected size, or the final block ends short of it */
#define DTK_INFLATE_S_ADLER 256    /* Adler-32 trailer mismatch (dtk_adler32) */
#define DTK_INFLATE_S_STREAM 512   /* a stream-table entry outside the buffers */
#define DTK_PNG_S_FILTER 1024      /* a filter byte > 4 (dtk_png_unfilter) */
int dtk_inflate(const uint8_t* in, int64_t in_bytes, const int64_t* streams, const int64_t* streams_host, int32_t n_streams,
                int32_t wrapper, uint8_t* out, int64_t out_bytes, int32_t* status, void* stream);
int dtk_adler32(const uint8_t* in, int64_t in_bytes, const int64_t* streams, const int64_t* streams_host, int32_t n_streams,
                const uint8_t* out, int64_t out_bytes, int32_t* status, void* stream);
size_t dtk_png_unfilter_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t bpp);
int dtk_png_unfilter(const uint8_t* raw, int32_t F, int32_t H, int32_t W, int32_t bpp, const uint8_t* lut, uint8_t* out,
                     int32_t* status, void* workspace, void* stream);

/* ---- Video and mask output: PNG ENCODING (docs/PNG_ENCODE.md): the PNG row filters, DEFLATE / zlib compression, the CRC-32 and whole
 * files; the mirror of the section above.  The filter stage, the Adler-32 and the CRC-32 are defined to the bit; the DEFLATE bytes are
 * a pure function of the input bytes and decode to them, but they are this library's, not zlib's. -----------------------------------
 * dtk_png_filter: frames uint8 [F][H][W][bpp], bpp = 1 or 3 -> raw [F][H][1 + W bpp], a filter byte and the filtered scanline per
 *   row: exactly what dtk_png_unfilter reads.  filter = 0 .. 4 (None, Sub, Up, Average, Paeth) forces that filter for every row;
 *   filter = 5 is adaptive: per row all five are computed and the one whose filtered bytes have the smallest sum of |value as int8|
 *   is taken, ties to the lowest filter number (the PNG specification's heuristic).  Encoding filters read ORIGINAL pixels: filtered
 *   = original - predictor mod 256, Average = floor((left + up) / 2), Paeth ties in the order left, up, up-left; bytes outside the
 *   image are 0.
 * dtk_deflate: the n_streams byte ranges of in [in_bytes] (ranges int64 [n_streams][DTK_DEFLATE_RANGE_FIELDS] = byte offset, byte
 *   length 0 .. 2^30) -> n_streams zlib streams (wrapper = 1: 78 01, DEFLATE data, the big-endian Adler-32 of the range) or raw DEFLATE
 *   streams (wrapper = 0), one after the other in out.  The table is passed twice, as in dtk_inflate: `ranges` on the device, and
 *   `ranges_host`, the same values in host memory, checked BEFORE anything is launched; the kernels repeat the check on their copy (an
 *   entry that does not fit is compressed as an empty range).  offsets int64 [n_streams + 1]: stream s is out[offsets[s] ..
 *   offsets[s + 1]); *needed (int64) = offsets[n_streams].  offsets and *needed are always written.  If *needed > out_capacity NOTHING
 *   is written to out and the call still returns 0: the caller reads *needed and calls again.  dtk_deflate_bound(n) is the longest
 *   stream n input bytes can give (n + 5 bytes per segment + 6), at most n + n / 1024 + 64: a capacity of its sum never needs a retry.
 *   Format: a range is cut into segments of DTK_DEFLATE_SEGMENT bytes (an empty range is one empty segment); one wave compresses a
 *   segment with no reference across its start, so every distance is <= 32768.  A segment is ONE block -- stored, fixed or dynamic
 *   Huffman, whichever is shortest by exact count (ties in that order) --; a coded block of a segment that is not the range's last is
 *   followed by an empty stored block (00 00 FF FF after the padding, zlib's sync flush), so every segment ends on a byte boundary;
 *   the last segment's block carries BFINAL.  Matches: greedy, lengths 3 .. 258, found among distance 1, two distances the caller
 *   of the PNG path names (a pixel, a row) and the newest position of an earlier 64-byte tile with the same 3-byte hash.  Dynamic
 *   codes: lengths limited to 15 (7 for the code-length code), literal/length and code-length codes complete, one distance code of
 *   length 1 when no match was emitted.
 *   workspace: dtk_deflate_workspace_bytes(ranges_host, n_streams) bytes, 256-byte aligned: per stream as many segments as the
 *   LONGEST range has, each a slot of DTK_DEFLATE_SEGMENT + 64 bytes and 4 DTK_DEFLATE_SEGMENT bytes of tokens -- about five times
 *   the input for ranges of one size.  0 for a null table, n_streams < 1 or a length outside 0 .. 2^30.
 * dtk_crc32: the CRC-32 of PNG and zlib (polynomial 0xEDB88320 reflected, start value and final xor 0xFFFFFFFF) of n_ranges byte
 *   ranges of data [data_bytes] -> crc uint32 [n_ranges].  ranges / ranges_host as above (lengths up to 2^40).  Table-driven over
 *   pieces of 64 bytes, which are combined by multiplication with x^(8 len) mod P.
 * dtk_png_encode: filter -> deflate -> assembly for frames uint8 [F][H][W][bpp].  header [33] (device): the caller's signature and
 *   IHDR chunk with its CRC, copied in front of every frame.  Each file is header, ONE IDAT chunk (length, "IDAT", the zlib stream,
 *   the CRC-32 over type and data) and IEND; the F files lie one after the other in out.  offsets [F + 1], *needed and out_capacity
 *   as in dtk_deflate; a file is at most 57 + dtk_deflate_bound(H (1 + W bpp)) bytes.  8-bit, non-interlaced, colour type 0 (bpp 1)
 *   or 2 (bpp 3).  workspace: dtk_png_encode_workspace_bytes(F, H, W, bpp) bytes, 256-byte aligned (the raw scanlines and
 *   dtk_deflate's workspace for them).
 * No host synchronisation inside.  Refused with DTK_E_INVALID before anything is launched: null pointers, F < 1, H or W < 1 or > 65535,
 *   bpp other than 1 / 3, more than 2^30 raw bytes per frame, filter outside 0 .. 5, in_bytes / data_bytes / n_streams / n_ranges < 1,
 *   wrapper other than 0 / 1, a ranges_host entry outside the buffer; dtk_png_encode_workspace_bytes returns 0 for such sizes. */
#define DTK_DEFLATE_SEGMENT 32768
#define DTK_DEFLATE_RANGE_FIELDS 2
#define DTK_PNG_FILTER_ADAPTIVE 5
int dtk_png_filter(const uint8_t* frames, int32_t F, int32_t H, int32_t W, int32_t bpp, int32_t filter, uint8_t* raw, void* stream);
int64_t dtk_deflate_bound(int64_t n);
size_t dtk_deflate_workspace_bytes(const int64_t* ranges_host, int32_t n_streams);
int dtk_deflate(const uint8_t* in, int64_t in_bytes, const int64_t* ranges, const int64_t* ranges_host, int32_t n_streams,
                int32_t wrapper, uint8_t* out, size_t out_capacity, int64_t* offsets, int64_t* needed, void* workspace, void* stream);
int dtk_crc32(const uint8_t* data, int64_t data_bytes, const int64_t* ranges, const int64_t* ranges_host, int32_t n_ranges,
              uint32_t* crc, void* stream);
size_t dtk_png_encode_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t bpp);
int dtk_png_encode(const uint8_t* frames, int32_t F, int32_t H, int32_t W, int32_t bpp, int32_t filter, const uint8_t* header,
                   uint8_t* out, size_t out_capacity, int64_t* offsets, int64_t* needed, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DTK_H_ */
