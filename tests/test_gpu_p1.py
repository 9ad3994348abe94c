"""-m gpu: DINOv2 ViT encoder (P1) through the C-ABI vs the fp32 oracle restatement (seeded random weights).
The device path uses fp16 matrix operands by default (fp32 accumulate / residual stream; bf16 on request), the oracle
fp32, so parity is stated at feature level, per-token cosine similarity and relative Frobenius error:
  * benchmark weights (LayerScale 0.1): cos >= 0.999999, rel <= 3e-4 (measured on MI355X: 1.1e-4 .. 1.4e-4; bf16: 1.0e-3);
  * LayerScale 1.0 (every block's update as large as the stream; the golden fixtures): rel <= 8e-4 (measured 3.2e-4 ..
    5.8e-4: each of the ~60 GEMM / attention stages adds ~2^-12 * sqrt(2) of relative operand rounding to an update that
    is not damped; bf16 sits at 2.5e-3 .. 4.5e-3 on the same inputs);
  * bf16 on request: cos >= 0.999, rel <= 2e-2."""
import pytest
import torch

from dino_tracker_amd import synth
from dino_tracker_amd.extractor import VitExtractor
from oracle import ref_algo as A

pytestmark = pytest.mark.gpu


BF16_TOL = dict(cos_min=0.999, rel_max=2e-2)
BENCH_TOL = dict(cos_min=0.999999, rel_max=3e-4)   # LayerScale 0.1 (what bench.py runs)


def _check(got, ref, cos_min=0.999999, rel_max=8e-4):
    got, ref = got.float().cpu(), ref.float().cpu()
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
    rel = (got - ref).norm() / ref.norm()
    assert cos.min() >= cos_min, (cos.min().item(), rel.item())
    assert rel <= rel_max, (cos.min().item(), rel.item())
    return cos.min().item(), rel.item()


@pytest.fixture(scope="module")
def vits():
    sd = synth.make_vit_weights("dinov2_vits14", seed=2)
    return sd, VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd)


@pytest.mark.parametrize("layer", [0, 3, 11])
def test_small_frames_all_depths(vits, layer):
    sd, ex = vits
    video = synth.synth_video(3, 140, 210, seed=71)  # 19 x 29 tokens; 3 frames in one batch
    feat = ex.encode(video, layer=layer)
    assert feat.shape == (3, 19 * 29, 384)
    for t in range(3):
        ref = A.vit_tokens(video[t:t + 1], sd, "dinov2_vits14", layer=layer).permute(1, 2, 0).reshape(-1, 384)
        _check(feat[t], ref)


@pytest.mark.parametrize("shape", [(3, 140, 210), (1, 98, 126), (2, 476, 854)])
def test_patch_embedding_is_fp32_grade(vits, shape):
    """layer = -1: tokens = patch embedding + position encoding, no block.  The split-fp16 MFMA kernel (hi + lo halves,
    three products; used when its scratch fits the workspace: the first and third shape) and the f32-input MFMA
    fallback (second shape) must both agree with an fp32 convolution to fp32 rounding level, not to bf16 level."""
    sd, ex = vits
    n, h, w = shape
    video = synth.synth_video(n, h, w, seed=77)
    feat = ex.encode(video, layer=-1)
    for t in range(n):
        ref = A.vit_tokens(video[t:t + 1].double(), {k: v.double() for k, v in sd.items()}, "dinov2_vits14",
                           layer=-1).permute(1, 2, 0).reshape(-1, 384)
        got = feat[t].double().cpu()
        rel = ((got - ref).norm() / ref.norm()).item()
        assert rel <= 2e-6, rel
        assert (got - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


def test_weight_stationary_gemm_matches_tiled_gemm():
    """The K = 384 GEMMs (QKV, projection, fc1) run on the weight-stationary kernel; dtk_vit_model.flags =
    DTK_VIT_TILED_GEMMS sends them to the tiled kernel instead.  Both use the same 16-bit operands, so after all 12 blocks the
    features must agree far more closely than either agrees with the fp32 oracle (differences: accumulation order, erf
    polynomial vs erff).  Run with the benchmark's LayerScale (0.1)."""
    sd = synth.make_vit_weights("dinov2_vits14", seed=2, layerscale=0.1)
    ex = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd)
    video = synth.synth_video(2, 140, 210, seed=78)
    a = ex.encode(video).cpu()
    ex.tiled_gemms = True
    b = ex.encode(video).cpu()
    assert not torch.equal(a, b)  # two different kernels did run
    _check(a, b, cos_min=0.999999, rel_max=3e-4)


def test_full_resolution_first_blocks(vits):
    """476 x 854 -> 8107 patch tokens + CLS (not a multiple of the 64-key tile: exercises the masked tail)."""
    sd, ex = vits
    video = synth.synth_video(1, 476, 854, seed=72)
    feat = ex.encode(video, layer=1)
    ref = A.vit_tokens(video, sd, "dinov2_vits14", layer=1).permute(1, 2, 0).reshape(-1, 384)
    _check(feat[0], ref)


def test_get_feature_from_input_includes_cls(vits):
    sd, ex = vits
    video = synth.synth_video(1, 98, 126, seed=73)
    m = torch.tensor(A.IMAGENET_MEAN).view(1, 3, 1, 1)
    s = torch.tensor(A.IMAGENET_STD).view(1, 3, 1, 1)
    tok = ex.get_feature_from_input(((video - m) / s).cuda(), layers=[2])
    assert tok.shape == (1, 1 + 13 * 17, 384)
    ref = A.vit_tokens(video, sd, "dinov2_vits14", layer=2).permute(1, 2, 0).reshape(-1, 384)
    _check(tok[0, 1:], ref)
    assert torch.isfinite(tok[0, 0]).all() and tok[0, 0].abs().sum() > 0


def test_get_dino_features_video_contract(vits):
    from dino_tracker_amd.utils import get_dino_features_video
    sd, _ = vits
    video = synth.synth_video(2, 98, 126, seed=74)
    out = get_dino_features_video(video.cuda(), model_name="dinov2_vits14", facet="tokens", stride=7, layer=1,
                                  device="cuda:0", state_dict=sd)
    assert out.device.type == "cpu" and out.shape == (2, 384, 13, 17)  # utils.py:53,67: T x C x ph x pw on the CPU
    ref = A.vit_tokens(video[1:2], sd, "dinov2_vits14", layer=1)
    _check(out[1].permute(1, 2, 0).reshape(-1, 384), ref.permute(1, 2, 0).reshape(-1, 384))


def test_vitb_width(vits):
    """ViT-B/14 (D = 768, 12 heads) shares the kernels."""
    sd = synth.make_vit_weights("dinov2_vitb14", seed=5)
    ex = VitExtractor("dinov2_vitb14", stride=7, device="cuda:0", state_dict=sd)
    video = synth.synth_video(1, 98, 126, seed=75)
    feat = ex.encode(video, layer=1)
    ref = A.vit_tokens(video, sd, "dinov2_vitb14", layer=1).permute(1, 2, 0).reshape(-1, 768)
    _check(feat[0], ref)


def test_attention_large_logits_force_rescale():
    """Online-softmax deferred-maximum branch: with 6x larger q/k projections the scores spread over tens of log2
    units, so the running maximum is overtaken by more than 8 many times along the key sweep (with the default weights
    the rescale only happens on the first tile).  The first block's output must still match the fp32 oracle."""
    sd = {k: v.clone() for k, v in synth.make_vit_weights("dinov2_vits14", seed=9).items()}
    d = 384
    sd["blocks.0.attn.qkv.weight"][:2 * d] *= 6.0  # q and k rows
    ex = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd)
    video = synth.synth_video(1, 238, 322, seed=76)  # 33 x 45 = 1485 tokens: 24 key tiles
    feat = ex.encode(video, layer=0)
    ref = A.vit_tokens(video, sd, "dinov2_vits14", layer=0).permute(1, 2, 0).reshape(-1, d)
    # 16-bit Q / K move a score by ~2^-11 |s| (|s| reaches tens here), i.e. P by a few 1e-3 relative
    _check(feat[0], ref, cos_min=0.9999, rel_max=5e-3)


# ---- against the un-modified reference extractor (tests/golden/p1_small.npz, written by make_golden.py) -----------------
def _gold():
    import os
    import numpy as np
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p1_small.npz"))


@pytest.mark.parametrize("tag,ls", [("ls1", 1.0), ("ls01", 0.1)])
def test_tokens_match_reference_extractor_golden(tag, ls):
    """utils.get_dino_features_video (reference signature) on the device vs the reference's own extractor code run on
    the DINOv2-API stub; layer=None = last block.  bf16 operand tolerance, stated per token."""
    import make_golden as MG
    from dino_tracker_amd.utils import get_dino_features_video
    gold = torch.from_numpy(_gold()[f"tokens_{tag}_l11"])
    video = MG.p1_video()[:gold.shape[0]]
    out = get_dino_features_video(video.cuda(), model_name=MG.P1_CASE["model"], facet="tokens", stride=7, layer=None,
                                  device="cuda:0", state_dict=MG.p1_weights(ls))
    assert out.shape == gold.shape and out.device.type == "cpu"
    for t in range(gold.shape[0]):
        cos, rel = _check(out[t].permute(1, 2, 0).reshape(-1, 384), gold[t].permute(1, 2, 0).reshape(-1, 384),
                          **(BENCH_TOL if ls == 0.1 else {}))
        print(f"tokens {tag} frame {t}: min cos {cos:.6f} rel {rel:.2e}")


def test_cls_row_and_layer_mean_match_reference_golden():
    """get_feature_from_input(img, [2, 5]): mean over two hooked layers, CLS row included (models/extractor.py:137-150)."""
    import make_golden as MG
    gold = torch.from_numpy(_gold()["feature_with_cls_l2_l5"])
    ex = VitExtractor(MG.P1_CASE["model"], stride=7, device="cuda:0", state_dict=MG.p1_weights(1.0))
    m = torch.tensor(A.IMAGENET_MEAN).view(1, 3, 1, 1)
    s = torch.tensor(A.IMAGENET_STD).view(1, 3, 1, 1)
    x = ((MG.p1_video()[:1] - m) / s).cuda()
    tok = ex.get_feature_from_input(x, layers=[2, 5]).cpu()
    assert tok.shape == gold.shape
    _check(tok[0], gold[0])
    cls_err = (tok[0, 0] - gold[0, 0]).norm() / gold[0, 0].norm()
    assert cls_err < 1e-3, cls_err  # the CLS token itself, not just "finite"
    # round 6: the multi-layer mean comes out of ONE pass (dtk_vit_model.tap_out) -- the same numbers as one pass per layer, for
    # fast blocks (the pending 16-bit update joins the tap), split blocks, and a mix of both
    for pr in ("fast", "split", [0, 3, 5]):
        e2 = VitExtractor(MG.P1_CASE["model"], stride=7, device="cuda:0", state_dict=MG.p1_weights(1.0), precision=pr)
        one = e2.get_feature_from_input(x, layers=[2, 5, 3])
        per = torch.stack([e2.encode(x, layer=l, normalize=False, want="tokens") for l in (2, 5, 3)]).mean(dim=0)
        assert (one - per).abs().max() <= 2e-6 * per.abs().max(), (pr, (one - per).abs().max().item())


def test_qkv_facets_match_reference_golden():
    """a4: qkv record, key facet through utils.get_dino_features_video(facet='keys'), key self-similarity."""
    import make_golden as MG
    from dino_tracker_amd.utils import get_dino_features_video
    g = _gold()
    sd = MG.p1_weights(1.0)
    ex = VitExtractor(MG.P1_CASE["model"], stride=7, device="cuda:0", state_dict=sd)
    m = torch.tensor(A.IMAGENET_MEAN).view(1, 3, 1, 1)
    s = torch.tensor(A.IMAGENET_STD).view(1, 3, 1, 1)
    video = MG.p1_video()[:1]
    x = ((video - m) / s).cuda()
    qkv = ex.get_qkv_feature_from_input(x)
    assert len(qkv) == 12
    _check(qkv[1][0].cpu(), torch.from_numpy(g["qkv_l1"])[0], cos_min=0.99999, rel_max=1e-3)
    keys = get_dino_features_video(video.cuda(), model_name=MG.P1_CASE["model"], facet="keys", stride=7, layer=3,
                                   device="cuda:0", state_dict=sd)
    gk = torch.from_numpy(g["keys_l3"])
    assert keys.shape == gk.shape
    _check(keys[0].permute(1, 2, 0).reshape(-1, 384), gk[0].permute(1, 2, 0).reshape(-1, 384), cos_min=0.99999, rel_max=1e-3)
    q = ex.get_queries_from_input(x, layers=[1])
    v = ex.get_values_from_input(x, layers=[1])
    gq = torch.from_numpy(g["qkv_l1"]).reshape(1, 222, 3, 384)
    _check(q[0].cpu(), gq[0, :, 0], cos_min=0.99999, rel_max=1e-3)
    _check(v[0].cpu(), gq[0, :, 2], cos_min=0.99999, rel_max=1e-3)
    ssim = ex.get_keys_self_sim_from_input(x, layer_num=1).cpu()
    assert (ssim - torch.from_numpy(g["keys_self_sim_l1"])).abs().max() < 2e-3
    attn = ex.get_attn_feature_from_input(x)[1]
    assert attn.shape == (1, 6, 222, 222) and (attn.sum(-1) - 1).abs().max() < 1e-4
    ref_attn = torch.softmax((gq[:, :, 0].reshape(1, 222, 6, 64).permute(0, 2, 1, 3) * 0.125)
                             @ gq[:, :, 1].reshape(1, 222, 6, 64).permute(0, 2, 3, 1), dim=-1)
    assert (attn.cpu() - ref_attn).abs().max() < 1e-3


def test_full_resolution_all_blocks_bench_weights():
    """476 x 854, all 12 blocks, the benchmark's weights (LayerScale 0.1) vs the fp32 oracle: the feature-level error
    of the bf16 path on exactly what bench.py runs (one frame; the oracle's ViT costs ~1.6 TFLOP on the host)."""
    sd = synth.make_vit_weights("dinov2_vits14", seed=2, layerscale=0.1)
    ex = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd)
    video = synth.synth_video(1, 476, 854, seed=2000)
    feat = ex.encode(video)
    ref = A.vit_tokens(video, sd, "dinov2_vits14").permute(1, 2, 0).reshape(-1, 384)
    cos, rel = _check(feat[0], ref, **BENCH_TOL)
    print(f"full-res 12 blocks, bench weights: min token cos {cos:.6f}, rel Frobenius {rel:.3e}")


@pytest.mark.parametrize("kernel", ["v6", "v4"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_attention_guards_and_safe_pass(dt, kernel):
    """dtk_vit_attention alone on crafted 16-bit operands vs an fp64 softmax on the SAME operands, for both operand types and
    both kernels (v6: the library's kernel since round 6, vit_attention6.h -- one wave per SIMD, FOUR query tiles per wave, every
    matrix instruction an asm statement on AGPR fragments, a tile's rescale deferred to the sub-step that issues its next PV
    product; v4: the one-wave-per-SIMD kernel of rounds 4-5, vit_attention4.h -- its reference enters through the
    MFMA's C operand and its two query tiles are guarded half a key tile apart, the fallback / cross-check).
    The kernel exponentiates scores optimistically against a reference it estimates once from the first 64 keys and the
    query tile's own 32 keys (csrc/vit_attention_common.h, "the guard arithmetic"); the rows below force every branch of that logic: (5) scores up to +-60 ->
    tile row sums beyond RESC_T -> power-of-two rescale of O / l, or beyond POISON_T -> safe pass (fp16: 2^9 / 2^15, bf16:
    2^40 / 2^120); (6) scores of +-300 -> poisoned sum -> safe pass; (7) about -300 for EVERY key -> an estimate far
    below 0; (8) a row whose large scores all sit in LATE tiles: the estimate is low and the sums jump past POISON_T in one
    step (fp16); and ordinary rows that share their wave with them.  S is not a multiple of the 64-key tile (masked tail)."""
    import vit_attention_ref as R
    from dino_tracker_amd import ops
    from dino_tracker_amd._lib import OPERAND_ATTENTION_V4, OPERAND_BF16, OPERAND_F16, check, lib
    tdt = torch.float16 if dt == "fp16" else torch.bfloat16
    g = torch.Generator().manual_seed(11)
    F, Hh, S = 1, 2, 1000
    Sp = 1024
    qs = 0.125 * 1.4426950408889634
    q = torch.zeros(F, Hh, Sp, 64)
    k = torch.zeros(F, Hh, Sp, 64)
    v = torch.zeros(F, Hh, Sp, 64)
    q[:, :, :S] = torch.randn(F, Hh, S, 64, generator=g) * qs * 1.5
    k[:, :, :S] = torch.randn(F, Hh, S, 64, generator=g)
    v[:, :, :S] = torch.randn(F, Hh, S, 64, generator=g)
    k[0, 0, :S, 0] += 50.0
    q[0, 0, 5] *= 25.0
    q[0, 0, 6] *= 120.0
    q[0, 0, 7] *= 0.01
    q[0, 0, 7, 0] = -6.0
    q[0, 1, 700] *= 120.0   # a poisoned row in another wave / head, late in the sweep
    # (8) head 1, row 300: channel 1 of the keys 640.. is large and the query looks along it: scores ~ +40 there, ~0 before
    k[0, 1, 640:S, 1] += 20.0
    q[0, 1, 300] *= 0.05
    q[0, 1, 300, 1] = 2.0
    qb, kb, vb = q.to(tdt), k.to(tdt), v.to(tdt)
    vt = vb.transpose(2, 3).contiguous()  # [F][H][64][Sp]
    out = torch.empty(F, S, Hh * 64, dtype=tdt, device="cuda")
    qd, kd, vd = qb.cuda().contiguous(), kb.cuda().contiguous(), vt.cuda().contiguous()
    check(lib().dtk_vit_attention(ops._p(qd), ops._p(kd), ops._p(vd), ops._p(out), F, Hh, S, Sp,
                                  (OPERAND_F16 if dt == "fp16" else OPERAND_BF16) | (OPERAND_ATTENTION_V4 if kernel == "v4" else 0),
                                  ops._stream()))
    s = R.scores(qb, kb, S)                                                      # exp2-domain scores
    ref = R.reference(qb, kb, vb, S)
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    rel = R.row_rel(got, ref)[0]
    # 16-bit P and 16-bit output: 2^-8 (bf16) / 2^-11 (fp16) of the row's largest output, every row, incl. the crafted ones
    tol = 6e-3 if dt == "bf16" else 1e-3
    assert rel.max() < tol, (int(rel.argmax()), rel.max().item())
    # the crafted rows really are extreme: near one-hot / far from the reference 0
    assert s[0, 0, 6].abs().max() > 200 and s[0, 0, 7].max() < -150 and s[0, 0, 5].abs().max() > 45
    assert s[0, 1, 300, 640:].min() > 30 and s[0, 1, 300, :96].max() < 8


def test_encoder_on_the_previous_attention_kernel_agrees(vits):
    """Round 6 moved dtk_vit_forward's attention to vit_attention6.h (four query tiles per wave); DTK_VIT_ATTENTION_V4 keeps rounds
    4-5's kernel (two tiles) selectable: both encoders against the fp32 oracle and against each other (the two kernels estimate the
    same per-query reference and differ in nothing but the order of the row sums), at a token count that is not a multiple of 128."""
    sd, ex = vits
    ex4 = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd)
    ex4.attention_v4 = True
    video = synth.synth_video(2, 238, 322, seed=83)     # 33 x 45 + 1 = 1486 tokens
    a, b = ex.encode(video, layer=5).cpu(), ex4.encode(video, layer=5).cpu()
    for t in range(2):
        ref = A.vit_tokens(video[t:t + 1], sd, "dinov2_vits14", layer=5).permute(1, 2, 0).reshape(-1, 384)
        _, ra = _check(a[t], ref)
        _, rb = _check(b[t], ref)
        assert abs(ra - rb) < 0.2 * max(ra, rb), (ra, rb)
    d = float((a - b).norm() / b.norm())
    print("attention6 vs attention4 encoders: rel", d)
    assert d < 2e-4, d


@pytest.mark.parametrize("path", ["v6", "v4", "split"])
def test_one_key_tile_frames_through_the_encoder(vits, path):
    """56 x 70 at stride 7: 7 x 9 patches + CLS = 64 tokens = exactly ONE 64-key tile with no masked tail (every other encoder test
    has at least four key tiles and a partial last one; the stage alone: tests/test_gpu_vit_attention_shapes.py), and every GEMM at 64
    rows per frame; two frames.  The default attention kernel and attention_v4 against the fp32 oracle at _check's default bounds,
    precision="split" against the float64 oracle at the bounds of test_gpu_precision.py::test_split_precision_is_fp32_grade."""
    sd, ex = vits
    video = synth.synth_video(2, 56, 70, seed=85)
    if path == "split":
        ex = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, precision="split")
    elif path == "v4":
        ex = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd)
        ex.attention_v4 = True
    feat = ex.encode(video, layer=1)
    assert feat.shape == (2, 7 * 9, 384) and torch.isfinite(feat).all()
    for t in range(2):
        if path == "split":
            ref = A.vit_tokens(video[t:t + 1].double(), {k: v.double() for k, v in sd.items()}, "dinov2_vits14",
                               layer=1).permute(1, 2, 0).reshape(-1, 384)
            got = feat[t].double().cpu()
            rel = ((got - ref).norm() / ref.norm()).item()
            tok_rel = ((got - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()
            print(f"64 tokens, split, frame {t}: rel {rel:.2e}, worst token {tok_rel:.2e}")
            assert rel < 2e-6 and tok_rel < 4e-6, (rel, tok_rel)
        else:
            ref = A.vit_tokens(video[t:t + 1], sd, "dinov2_vits14", layer=1).permute(1, 2, 0).reshape(-1, 384)
            cos, rel = _check(feat[t], ref)
            print(f"64 tokens, {path}, frame {t}: min cos {cos:.7f}, rel {rel:.2e}")


# ---- operand types and the fp16 range ---------------------------------------------------------------------------------
def test_bf16_operands_on_request(vits):
    """operand_dtype='bf16' (DTK_VIT_BF16): the round-2 arithmetic, kept for activations beyond fp16's range."""
    sd, ex16 = vits
    exb = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, operand_dtype="bf16")
    video = synth.synth_video(2, 140, 210, seed=79)
    a, b = ex16.encode(video).cpu(), exb.encode(video).cpu()
    assert not torch.equal(a, b)
    for t in range(2):
        ref = A.vit_tokens(video[t:t + 1], sd, "dinov2_vits14").permute(1, 2, 0).reshape(-1, 384)
        c16, r16 = _check(a[t], ref)
        cb, rb = _check(b[t], ref, **BF16_TOL)
        print(f"frame {t}: fp16 rel {r16:.2e}, bf16 rel {rb:.2e}")
        assert r16 < 0.4 * rb  # fp16 operands are what buys the end-to-end 1e-3 px


def _outlier_weights(scale_fc2=1.0):
    """ViT-S weights with DINOv2-like statistics (massive activations, large gains, a sharp block, a large MLP output):
    dino_tracker_amd.synth.make_outlier_vit_weights (bit-identical to the generator that lived here in rounds 3-5)."""
    return synth.make_outlier_vit_weights(scale_fc2)


def test_outlier_tokens_stay_in_fp16_range():
    """1e3-scale outlier tokens in the fp32 residual stream, large gains, a peaked-attention block and an MLP whose output is
    ~1e3: every 16-bit tensor must stay finite and un-saturated (overflow word 0, also with the full range scan) and the
    features must match the fp32 oracle at the fp16 tolerance relative to the token norms."""
    sd = _outlier_weights(scale_fc2=300.0)
    ex = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, check_range=True)
    video = synth.synth_video(2, 238, 322, seed=80)
    tok = ex.encode(video, layer=5, want="tokens").cpu()
    assert ex.last_overflow == 0 and torch.isfinite(tok).all()
    for t in range(2):
        ref = A.vit_tokens(video[t:t + 1], sd, "dinov2_vits14", layer=5)
        ref = ref.permute(1, 2, 0).reshape(-1, 384)
        assert ref.abs().max() > 500  # the outliers are there
        # 16-bit Q / K move a score by ~2^-12 |s| and |s| reaches 100 here (P by percents for the sharpest rows): measured
        # rel 2.1e-3 / min cos 0.99997 with fp16 operands; the same inputs with bf16 operands are 8x further away
        cos, rel = _check(tok[t, 1:], ref, cos_min=0.9999, rel_max=4e-3)
        print(f"outlier frame {t}: max |x| {ref.abs().max().item():.0f}, min cos {cos:.7f}, rel {rel:.2e}")
    exb = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, operand_dtype="bf16")
    tokb = exb.encode(video[:1], layer=5, want="tokens").cpu()
    ref0 = A.vit_tokens(video[:1], sd, "dinov2_vits14", layer=5).permute(1, 2, 0).reshape(-1, 384)
    relb = ((tokb[0, 1:] - ref0).norm() / ref0.norm()).item()
    rel16 = ((tok[0, 1:] - ref0).norm() / ref0.norm()).item()
    print(f"outlier frame 0: fp16 rel {rel16:.2e}, bf16 rel {relb:.2e}")
    assert rel16 < 0.4 * relb


def test_fp16_saturation_is_reported_and_bf16_is_the_way_out():
    """An MLP output beyond 65504 cannot be an fp16 residual update: the device saturates it (no inf / NaN downstream) and
    sets the overflow word.  on_overflow="raise": `encode` raises naming operand_dtype='bf16'.  on_overflow="bf16" (round 5's
    default, opt-in since round 6): the call is re-encoded on plain bf16 operands -- bit-identical to an extractor built with
    operand_dtype="bf16" --, counted, and the extractor stays on bf16.  The round-6 default (split bf16) is in
    tests/test_gpu_precision.py."""
    sd = _outlier_weights(scale_fc2=3.0e5)
    video = synth.synth_video(1, 140, 210, seed=81)
    ex = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, on_overflow="raise")
    with pytest.raises(RuntimeError, match="operand_dtype='bf16'"):
        ex.encode(video, layer=4)
    assert ex.last_overflow & 1
    exb = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, operand_dtype="bf16")
    feat = exb.encode(video, layer=4).cpu()
    ref = A.vit_tokens(video, sd, "dinov2_vits14", layer=4).permute(1, 2, 0).reshape(-1, 384)
    assert torch.isfinite(feat).all()
    _check(feat[0], ref, **BF16_TOL)
    exh = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, on_overflow="bf16")
    with pytest.warns(RuntimeWarning, match="bf16"):
        healed = exh.encode(video, layer=4).cpu()
    assert exh.range_fallbacks == 1 and exh.operand_dtype == "bf16" and exh.last_overflow == 0
    assert torch.equal(healed, feat)
    assert torch.equal(exh.encode(video, layer=4).cpu(), feat) and exh.range_fallbacks == 1   # sticky: no second fp16 attempt
    # a deferred check cannot heal (the features were handed on): it raises, and the extractor is on bf16 afterwards
    exd = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, on_overflow="bf16")
    exd.encode(video, layer=4, defer_check=True)
    with pytest.warns(RuntimeWarning), pytest.raises(RuntimeError, match="deferred"):
        exd.check_overflow()
    assert exd.operand_dtype == "bf16" and torch.equal(exd.encode(video, layer=4).cpu(), feat)
    # a deferred saturating call FOLLOWED by a non-deferred call -- the word's bits cannot be attributed to the
    # current call, so encode's own check must not "heal" (re-run only the current call and hand the earlier saturated
    # features on silently): it raises the deferred error
    exq = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, on_overflow="bf16")
    exq.encode(video, layer=4, defer_check=True)
    with pytest.warns(RuntimeWarning), pytest.raises(RuntimeError, match="deferred"):
        exq.encode(video, layer=4)
    assert exq.operand_dtype == "bf16" and exq.last_overflow & 1
    assert torch.equal(exq.encode(video, layer=4).cpu(), feat)   # afterwards: a clean bf16 extractor


def _late_frame_saturation_case(which):
    """ViT-S weights + a 40-frame clip in which ONLY frame 37 drives one value past the fp16 limit: `which` = "hidden" (one unit
    of block 0's MLP hidden, overflow bit 4) or "qkv" (one key channel of block 0, bit 2).  Frames 0..36, 38, 39 are the same
    dark image, frame 37 a bright one; the planted unit reads the difference of the two frames' LayerNorm outputs (computed
    with the oracle on the CPU), so it is ~0 on the dark frames and ~1e5 on the bright one.  Rounds 3-4 scanned frame 0 only."""
    T, H, W = 40, 98, 126
    sd = {k: v.clone() for k, v in synth.make_vit_weights("dinov2_vits14", seed=21, layerscale=0.1).items()}
    dark = 0.2 + 0.02 * torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(1))
    bright = 0.8 + 0.02 * torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(2))
    video = dark.repeat(T, 1, 1, 1)
    video[37] = bright[0]

    def ln_out(frame, norm):   # LayerNorm output that feeds block 0's qkv (norm1) / fc1 (norm2), all tokens
        tok = A.vit_all_tokens(frame, sd, "dinov2_vits14", layer=-1 if norm == "norm1" else 0)
        if norm == "norm2":    # x after the attention half of block 0 = what norm2 sees: recompute it from the block's definition
            x0 = A.vit_all_tokens(frame, sd, "dinov2_vits14", layer=-1)
            y = torch.nn.functional.layer_norm(x0, (384,), sd["blocks.0.norm1.weight"], sd["blocks.0.norm1.bias"], eps=1e-6)
            qkv = torch.nn.functional.linear(y, sd["blocks.0.attn.qkv.weight"], sd["blocks.0.attn.qkv.bias"]).reshape(1, -1, 3, 6, 64)
            q, k, v = qkv.permute(2, 0, 3, 1, 4)
            a = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(1, -1, 384)
            tok = x0 + sd["blocks.0.ls1.gamma"] * torch.nn.functional.linear(a, sd["blocks.0.attn.proj.weight"], sd["blocks.0.attn.proj.bias"])
        return torch.nn.functional.layer_norm(tok, (384,), sd[f"blocks.0.{norm}.weight"], sd[f"blocks.0.{norm}.bias"], eps=1e-6)[0]

    norm = "norm2" if which == "hidden" else "norm1"
    yd, yb = ln_out(dark, norm), ln_out(bright, norm)
    d = yb.mean(0) - yd.mean(0)
    pd, pb = yd @ d, yb @ d                                 # every token's coordinate along the dark -> bright direction
    sc = 7.0e4 / float(pb.max() - pd.max())                 # the largest dark token lands on 3e4, the largest bright one on 1e5
    w = sc * d
    b = 3.0e4 - sc * float(pd.max())
    assert w.abs().max() < 3.0e4, w.abs().max()            # the planted weights themselves fit fp16
    vals_d, vals_b = yd @ w + b, yb @ w + b
    assert vals_d.abs().max() < 4.5e4 and vals_b.max() > 9.0e4, (vals_d.abs().max(), vals_b.max())
    if which == "hidden":
        sd["blocks.0.mlp.fc1.weight"][5] = w
        sd["blocks.0.mlp.fc1.bias"][5] = b
        sd["blocks.0.mlp.fc2.weight"][:, 5] = 0.0           # keep the residual update itself in range: only bit 4 may fire
    else:
        sd["blocks.0.attn.qkv.weight"][384 + 70] = w        # key channel 6 of head 1
        sd["blocks.0.attn.qkv.bias"][384 + 70] = b
    return sd, video


@pytest.mark.parametrize("which,bit", [("hidden", 4), ("qkv", 2)])
def test_saturation_in_a_late_frame_is_caught_and_healed(which, bit):
    """Q / K / V and the MLP hidden are range-checked for EVERY frame inside the GEMM epilogues (no extra
    pass) -- a clip whose frame 37 alone saturates is reported (on_overflow="raise"), agrees with the explicit scan
    (check_range=True), and with on_overflow="bf16" is re-encoded on bf16 operands (the round-6 default, split bf16:
    tests/test_gpu_precision.py)."""
    sd, video = _late_frame_saturation_case(which)
    ex = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, on_overflow="raise")
    ex.encode(video[:37], layer=1)                          # the dark frames alone: in range
    assert ex.last_overflow == 0
    with pytest.raises(RuntimeError, match="fp16 range"):
        ex.encode(video, layer=1)
    assert ex.last_overflow & bit, ex.last_overflow
    exs = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, on_overflow="raise", check_range=True)
    with pytest.raises(RuntimeError):
        exs.encode(video, layer=1)
    assert exs.last_overflow & bit
    ext = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, on_overflow="raise")
    ext.tiled_gemms = True                                  # the generic GEMM kernels' epilogues track the range too
    with pytest.raises(RuntimeError):
        ext.encode(video, layer=1)
    assert ext.last_overflow & bit
    exh = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, on_overflow="bf16")
    with pytest.warns(RuntimeWarning):
        healed = exh.encode(video, layer=1).cpu()
    exb = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd, operand_dtype="bf16")
    assert exh.range_fallbacks == 1 and torch.equal(healed, exb.encode(video, layer=1).cpu())
    assert torch.isfinite(healed).all()
    if which == "hidden":   # (a key channel of 1e5 makes the attention a near-one-hot lottery at ANY 16-bit key rounding: no oracle bound there)
        ref = A.vit_tokens(video[37:38], sd, "dinov2_vits14", layer=1).permute(1, 2, 0).reshape(-1, 384)
        _check(healed[37], ref, **BF16_TOL)


def test_weights_from_an_upstream_named_checkpoint_file(tmp_path, monkeypatch):
    """$DTK_DINOV2_WEIGHTS (extractor.py: the path torch.hub's dinov2_vits14_pretrain.pth would take; models/extractor.py:23-39
    loads the hub model): a state dict in upstream naming WITH the keys the encoder does not use (`mask_token`, the final
    `norm.*`, a `pos_embed` of 1 x 1370 x D) loads, and encodes exactly like the same weights passed as `state_dict=`."""
    sd = synth.make_vit_weights("dinov2_vits14", seed=31, layerscale=0.1)
    assert sd["pos_embed"].shape == (1, 1370, 384)
    full = dict(sd)
    full["mask_token"] = torch.zeros(1, 384)
    full["norm.weight"], full["norm.bias"] = torch.ones(384), torch.zeros(384)
    path = str(tmp_path / "dinov2_vits14_pretrain.pth")
    torch.save(full, path)
    video = synth.synth_video(2, 140, 210, seed=84)
    want = VitExtractor("dinov2_vits14", stride=7, device="cuda:0", state_dict=sd).encode(video).cpu()
    monkeypatch.setenv("DTK_DINOV2_WEIGHTS", path)
    got = VitExtractor("dinov2_vits14", stride=7, device="cuda:0").encode(video).cpu()
    assert torch.equal(got, want)
    monkeypatch.delenv("DTK_DINOV2_WEIGHTS")
    with pytest.raises(RuntimeError, match="no DINOv2 weights"):
        VitExtractor("dinov2_vits14", stride=7, device="cuda:0")


# ---- ViT-L/14: the reference's shipped configuration (config/preprocessing.yaml:10-13), no reference checkout needed --------
def test_vitl_layer15_full_resolution_and_all_24_blocks():
    """dinov2_vitl14 (D = 1024, 16 heads, K = 1024 / 4096 GEMMs on gemm_wide_kernel): one 476 x 854 synthetic frame to the
    hooked block 15 -- what preprocessing/save_dino_embed_video.py computes per frame -- and one small frame through all
    24 blocks, against the fp32 oracle."""
    sd = synth.make_vit_weights("dinov2_vitl14", seed=6, layerscale=0.1)
    ex = VitExtractor("dinov2_vitl14", stride=7, device="cuda:0", state_dict=sd)
    video = synth.synth_video(1, 476, 854, seed=82)
    feat = ex.encode(video, layer=15).cpu()
    assert feat.shape == (1, 67 * 121, 1024)
    ref = A.vit_tokens(video, sd, "dinov2_vitl14", layer=15).permute(1, 2, 0).reshape(-1, 1024)
    cos, rel = _check(feat[0], ref, rel_max=5e-4)  # 16 blocks, K = 1024 / 4096 (measured 3.4e-4)
    print(f"ViT-L block 15 at 476x854: min token cos {cos:.7f}, rel {rel:.2e}")
    small = synth.synth_video(2, 140, 210, seed=83)
    tok = ex.encode(small, want="tokens").cpu()  # layer None = 23
    for t in range(2):
        r = A.vit_tokens(small[t:t + 1], sd, "dinov2_vitl14").permute(1, 2, 0).reshape(-1, 1024)
        cos, rel = _check(tok[t, 1:], r, rel_max=6e-4)
        print(f"ViT-L 24 blocks, frame {t}: min token cos {cos:.7f}, rel {rel:.2e}")


@pytest.mark.parametrize("name,layer", [("dinov2_vits14", 2), ("dinov2_vitb14", 3), ("dinov2_vitl14", 2)])
def test_wide_gemm_fragment_prefetch_is_bit_identical(name, layer):
    """Round 6: gemm_wide_kernel (D = 768 / 1024) reads its fragments one half-step ahead of the MFMAs that consume them and its
    stages arrive through buffer descriptors; every accumulator still sums its k-steps in the same order, so the features are
    BIT-identical to the round 4-5 loop (DTK_VIT_GEMM_WIDE_V1), here over a frame whose token count is not a multiple of the 256-row
    tile (clamped tail rows) and, against the tiled kernel (different tile shape, same k order per accumulator), close (the tiled epilogues differ in their GELU form)."""
    sd = synth.make_vit_weights(name, seed=9, layerscale=0.1)
    # 154 x 238: S = 694 tokens per frame (V^T leaves element by element); 140 x 154: S = 400, a multiple of 4 (V^T leaves as 8-byte
    # pieces of four tokens, the form of 854 x 476); three frames: tiles that cross a frame boundary, clamped tail rows
    for hw in ((154, 238), (140, 154)):
        video = synth.synth_video(3, hw[0], hw[1], seed=84)
        out = {}
        for form in ("new", "v1", "tiled"):
            ex = VitExtractor(name, stride=7, device="cuda:0", state_dict=sd)
            ex.gemm_wide_v1, ex.tiled_gemms = form == "v1", form == "tiled"
            out[form] = ex.encode(video, layer=layer)
        assert torch.isfinite(out["new"]).all()
        assert torch.equal(out["new"], out["v1"]), hw
        if name == "dinov2_vits14":   # the weight-stationary GEMMs vs their round 1-3 form; fc2 + the next block's LayerNorm vs two launches
            ex = VitExtractor(name, stride=7, device="cuda:0", state_dict=sd)
            ex.gemm_ws_v1 = True
            assert torch.equal(out["new"], ex.encode(video, layer=layer)), hw
            ex = VitExtractor(name, stride=7, device="cuda:0", state_dict=sd)
            ex.no_ln_fusion = True
            assert torch.equal(out["new"], ex.encode(video, layer=layer)), hw
            assert torch.equal(ex.encode(video, want="tokens"), VitExtractor(name, stride=7, device="cuda:0", state_dict=sd).encode(video, want="tokens")), hw
        rel = ((out["new"].double() - out["tiled"].double()).norm() / out["tiled"].double().norm()).item()
        print(f"{name} {hw}: wide vs tiled GEMMs rel {rel:.2e}")
        assert rel < 2e-4
