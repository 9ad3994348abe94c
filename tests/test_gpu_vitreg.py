"""-m gpu: DINOv2 with registers (dinov2_vit{s,b,l,g}14_reg) through the encoder and the public interface, against the float64
restatement of tests/vitreg_ref.py.  Token rows: CLS, four registers (no position encoding), the patches; S = 1 + 4 + ph * pw.

Weights: the first two blocks (one for the widths B / L / g) of synth.make_vit_weights(name, seed=9), LayerScale 1.0, and synth.synth_video
frames; cases and references are vitreg_ref.CASES / make_case, computed once per process on the CPU.  The shapes are chosen for the places
where four more rows can go wrong: 3 x 98 x 126 (S = 226: frame ends inside every row tile), 2 x 42 x 182 (S = 130: Sp goes from 128 to
256), 3 x 28 x 42 (S = 20 < 32 with several frames: the dispatch of docs/PARITY.md's finding (1)), 1 x 14 x 14 (S = 6).

Tolerances are the project's classes (vitreg_ref.FP16_TOL / BF16_TOL; split operands: <= 4 x the float32 restatement's own error), and
tests/test_vitreg_reference.py asserts that every case moves by >= 10 x the fast-fp16 class when its registers are removed.  The bf16 class
is wider than the whole effect of four tokens among 226 (1.3e-2), so the bf16 run of the main case does not guard the registers by itself;
the one-patch case (0.51) is run on bf16 as well.  The figures each test prints are recorded in docs/PARITY.md ("DINOv2 with registers")."""
import pytest
import torch

import vitreg_ref as V
from dino_tracker_amd import ops, synth
from dino_tracker_amd.extractor import VitExtractor
from dino_tracker_amd.utils import get_dino_features_video, get_dino_features_video_packed
from oracle import ref_algo as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PX_TOL = 1e-3       # identical features: tests/test_gpu_p3.py / test_gpu_bench_path.py


def _ex(c, sd=None, name=None, **kw):
    return VitExtractor(name or c["name"], stride=c["stride"], device=DEV, state_dict=c["sd"] if sd is None else sd, **kw)


def _records(ex, c, layer=None, records=("tokens", "feat", "qkv")):
    layer = c["layer"] if layer is None else layer
    return {k: ex.encode(c["video"], layer=layer, want=k) for k in records}


def _fmt(fig):
    return ", ".join(f"{k}: min cos {v[0]:.7f} rel {v[1]:.2e}" for k, v in fig.items())


# ---- exact: the embedding, both patch-embedding kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["main", "main14"], ids=["stride7-split-fp16", "stride14-generic"])
@pytest.mark.parametrize("frame_batch", [0, 2], ids=["one-pass", "two-passes"])
def test_embedding_rows_are_exact(key, frame_batch):
    """layer = -1 runs the patch embedding and the positions with no block.  Against the SAME extractor code on the plain sibling with the
    same weights: row 0 bit-equal, rows 1 .. 4 bit-equal to register_tokens, rows 5 .. bit-equal to the sibling's rows 1 ..; the features of
    that pass (the prefix-drop kernel) are rows 5 .. bit for bit.  frame_batch = 2: the third frame's prefix is written by a second pass."""
    c = V.make_case(key)
    ex, plain = _ex(c), _ex(c, sd=V.without_registers(c["sd"]), name=c["plain"])
    ex.frame_batch = plain.frame_batch = frame_batch
    tok = ex.encode(c["video"], layer=-1, want="tokens")
    ptok = plain.encode(c["video"], layer=-1, want="tokens")
    hw = ptok.shape[1] - 1
    assert tok.shape == (c["video"].shape[0], 1 + 4 + hw, 384)
    V.check_embedding_exact(tok, ptok, c["sd"]["register_tokens"])
    feat = ex.encode(c["video"], layer=-1, want="feat")
    assert feat.shape == (c["video"].shape[0], hw, 384) and torch.equal(feat, tok[:, 5:])
    # and the float64 restatement agrees with what was compared bit for bit (fp32-grade embedding on both kernels)
    ref = V.encode(c["video"].double(), c["sd64"], -1, c["heads"], stride=c["stride"])["tokens"]
    assert V.rel(tok, ref) <= 2e-6


# ---- the main case ------------------------------------------------------------------------------------------------------------------------
def test_main_fast_fp16_records_and_shapes():
    c = V.make_case("main")
    ex = _ex(c)
    assert ex.n_registers == 4 and ex.get_n_layers() == 12 and ex.n_blocks == 2 and ex.get_head_num() == 6
    got = _records(ex, c)
    assert got["tokens"].shape == (3, 226, 384) and got["feat"].shape == (3, 221, 384) and got["qkv"].shape == (3, 226, 1152)
    print("vitreg ViT-S fast fp16, block 1 --", _fmt(V.check_records(got, c["ref"][1], **V.FP16_TOL)))
    print("vitreg ViT-S fast fp16, block 0 --", _fmt(V.check_records(_records(ex, c, 0), c["ref"][0], **V.FP16_TOL)))
    assert ex.last_overflow == 0 and ex.range_fallbacks == 0
    # the features are the patch rows of the tokens of the same pass, bit for bit (the final-update kernel drops 1 + R rows)
    assert torch.equal(got["feat"], got["tokens"][:, 5:])


def test_main_taps_are_the_mean_of_the_single_layer_calls():
    c = V.make_case("main")
    ex = _ex(c)
    norm = (c["video"] - torch.tensor(A.IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.tensor(A.IMAGENET_STD).view(1, 3, 1, 1)
    both = ex.get_feature_from_input(norm, layers=[0, 1])
    singles = torch.stack([ex.get_feature_from_input(norm, layers=[l]) for l in (0, 1)]).mean(dim=0)
    assert both.shape == (3, 226, 384)
    r = V.rel(both, singles.cpu())
    print(f"vitreg taps [0, 1] vs the mean of the single-layer calls: rel {r:.2e}")
    assert r <= 2e-6     # (tests/test_gpu_vitg.py: the same fp32 sums in another order)
    V.check(both, c["ref"][1]["taps"], **V.FP16_TOL)


def test_main_fast_bf16():
    c = V.make_case("main")
    print("vitreg ViT-S fast bf16, block 1 --", _fmt(V.check_records(_records(_ex(c, operand_dtype="bf16"), c), c["ref"][1], **V.BF16_TOL)))


def test_main_split_is_fp32_grade():
    c = V.make_case("main")
    ex = _ex(c, precision="split")
    got = _records(ex, c)
    for k in ("tokens", "feat", "qkv"):
        r, r32 = V.check_split(got[k], c["ref"][1][k], c["ref32"][k])
        print(f"vitreg ViT-S split fp16, block 1, {k}: rel {r:.2e} (float32 restatement on the CPU: {r32:.2e})")
    assert ex.precision_report()["split_blocks"] == list(range(12))


def test_main_tiled_gemms_against_the_default():
    """DTK_VIT_TILED_GEMMS against the weight-stationary / LDS-DMA kernels on the same 16-bit operands (the figure of tests/test_gpu_p1.py and
    test_gpu_vitg.py for this comparison), and each against float64."""
    c = V.make_case("main")
    ex = _ex(c)
    a = _records(ex, c)
    ex.tiled_gemms = True
    b = _records(ex, c)
    for k in a:
        cos, r = V.check(a[k], b[k].cpu(), cos_min=0.999999, rel_max=3e-4)
        print(f"vitreg default vs tiled GEMMs, block 1, {k}: rel {r:.2e}, bit-equal {torch.equal(a[k], b[k])}")
    V.check_records(b, c["ref"][1], **V.FP16_TOL)


@pytest.mark.parametrize("precision", ["fast", "split"])
def test_main_frame_batch_two(precision):
    """Three frames at two frames per pass: the second pass writes its own prefix rows and its outputs land behind the first pass's."""
    c = V.make_case("main")
    ex = _ex(c, precision=precision)
    ex.frame_batch = 2
    got = _records(ex, c)
    if precision == "fast":
        print("vitreg frame_batch = 2, fast fp16 --", _fmt(V.check_records(got, c["ref"][1], **V.FP16_TOL)))
    else:
        for k in got:
            V.check_split(got[k], c["ref"][1][k], c["ref32"][k])
    norm = (c["video"] - torch.tensor(A.IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.tensor(A.IMAGENET_STD).view(1, 3, 1, 1)
    V.check(ex.get_feature_from_input(norm, layers=[0, 1]), c["ref"][1]["taps"], **V.FP16_TOL)


# ---- Sp boundary, short frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["sp", "short", "one"])
def test_boundary_shapes(key):
    """sp: S = 130, Sp = 256 where the plain model has 126 / 128 (one more key tile, all padding but two rows).  short: S = 20 < 32 with three
    frames (the qkv GEMM's dispatch for frames shorter than a row tile).  one: a single patch, S = 6 (bf16 as well: see the module docstring)."""
    c = V.make_case(key)
    n = c["video"].shape[0]
    hw = {"sp": 125, "short": 15, "one": 1}[key]
    ref = c["ref"][1]
    got = _records(_ex(c), c)
    assert got["tokens"].shape == (n, 5 + hw, 384) and got["qkv"].shape == (n, 5 + hw, 1152) and got["feat"].shape == (n, hw, 384)
    print(f"vitreg {key} fast fp16 --", _fmt(V.check_records(got, ref, **V.FP16_TOL)))
    gs = _records(_ex(c, precision="split"), c)
    for k in gs:
        r, r32 = V.check_split(gs[k], ref[k], c["ref32"][k])
        print(f"vitreg {key} split fp16, {k}: rel {r:.2e} (float32 restatement: {r32:.2e})")
    if key == "one":
        print("vitreg one fast bf16 --", _fmt(V.check_records(_records(_ex(c, operand_dtype="bf16"), c), ref, **V.BF16_TOL)))


# ---- widths -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["vitb", "vitl", "vitg"])
def test_widths_one_block(key):
    """One block of ViT-B / L / g (SwiGLU) with registers at the main shape, fast and split.  ViT-g sits AT the fp16 class already (7.99e-4
    for the plain model, tests/test_gpu_vitg.py), so its fast pass is held to the plain sibling instead: same weights, same frames, same
    test -- the register model's error <= 1.15 x the sibling's (five more tokens in 222 cannot change the rounding budget by more)."""
    c = V.make_case(key)
    d = synth.VIT_CONFIGS[c["name"]]["dim"]
    ref = c["ref"][0]
    ex = _ex(c)
    got = _records(ex, c, records=("tokens", "feat"))
    assert got["tokens"].shape == (3, 226, d) and got["feat"].shape == (3, 221, d)
    if key == "vitg":
        with torch.no_grad():
            pref = V.encode(c["video"].double(), V.without_registers(c["sd64"]), 0, c["heads"])
        pgot = _records(_ex(c, sd=V.without_registers(c["sd"]), name=c["plain"]), c, records=("tokens", "feat"))
        for k in ("tokens", "feat"):
            r, rp = V.rel(got[k], ref[k]), V.rel(pgot[k], pref[k])
            cos = torch.nn.functional.cosine_similarity(got[k].double().cpu(), ref[k], dim=-1).min().item()
            print(f"vitreg ViT-g fast fp16, block 0, {k}: rel {r:.3e} (plain sibling {rp:.3e}, ratio {r / rp:.3f}), min cos {cos:.7f}")
            assert r <= 1.15 * rp, (k, r, rp)
            assert cos >= V.FP16_TOL["cos_min"]
    else:
        print(f"vitreg {key} fast fp16, block 0 --", _fmt(V.check_records(got, ref, records=("tokens", "feat"), **V.FP16_TOL)))
    gs = _records(_ex(c, precision="split"), c, records=("tokens", "feat"))
    for k in gs:
        r, r32 = V.check_split(gs[k], ref[k], c["ref32"][k])
        print(f"vitreg {key} split fp16, block 0, {k}: rel {r:.2e} (float32 restatement: {r32:.2e})")


# ---- guards -------------------------------------------------------------------------------------------------------------------------------
def trained_like_registers(sd, heads=6, channel=7, amplitude=1000.0, gain=4.0, beta=16.0):
    """Registers as a trained model has them: a large norm carried by one channel, and keys that every query scores far above the patches.
    Scaling register_tokens alone cannot do that -- LayerNorm-1 removes the scale -- so: the registers get `amplitude` in `channel` (their
    normalised row is then ~sqrt(D) there and ~0 elsewhere), LayerNorm-1 of block 0 gets gain `gain` in that channel, and every head's query
    bias gets `beta` along that head's key column of the channel.  A register's score is then ~beta |w_k| sqrt(D) gain / 8 ~ 50 nats, a patch's a few."""
    sd = {k: v.clone() for k, v in sd.items()}
    d = sd["cls_token"].shape[-1]
    sd["register_tokens"][..., channel] = amplitude
    sd["blocks.0.norm1.weight"][channel] = gain
    wk = sd["blocks.0.attn.qkv.weight"][d:2 * d, channel].reshape(heads, 64)
    sd["blocks.0.attn.qkv.bias"][:d] = (beta * wk / wk.norm(dim=1, keepdim=True)).reshape(d)
    return sd


def test_attention_guards_with_dominant_register_keys():
    """The attention kernels estimate each query's reference from the first 64 keys, which hold CLS and the registers.  With registers whose
    keys give the row maximum far above every patch score (asserted on the float64 qkv record: >= 20 nats in every head of every query),
    block 0's softmax sits on the four register keys.  The output stays in the fast-fp16 class; observed on the MI355X: overflow word 0, no
    heal (range_fallbacks == 0) -- the estimate is the true maximum, no rescale or safe pass is needed.  Should a later kernel saturate here,
    the heal path must have been taken and counted."""
    c = V.make_case("main")
    sd = trained_like_registers(c["sd"])
    with torch.no_grad():
        r0 = V.encode(c["video"].double(), V.to64(sd), 0, c["heads"])
        ref = V.encode(c["video"].double(), V.to64(sd), 1, c["heads"])
    q, k, _ = r0["qkv"].reshape(3, 226, 3, 6, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) / 8.0                       # nats
    margin = float((s[..., 1:5].max(dim=-1).values - torch.cat([s[..., :1], s[..., 5:]], dim=-1).max(dim=-1).values).min())
    print(f"dominant registers: the best register score is >= {margin:.1f} nats above every other key's, over all queries and heads")
    assert margin >= 20.0
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # (the heal path warns; it is asserted through its counter below)
        ex = _ex(c, sd=sd)
        got = _records(ex, c, records=("feat", "qkv"))
    print(f"dominant registers: overflow word {ex.last_overflow}, range_fallbacks {ex.range_fallbacks}, operands {ex.operand_dtype} --",
          _fmt(V.check_records(got, ref, records=("feat", "qkv"), **V.FP16_TOL)))
    assert ex.last_overflow == 0
    assert ex.range_fallbacks == 0 or (ex.operand_dtype == "bf16" and len(ex.split_blocks) == 12)
    exv4 = _ex(c, sd=sd)
    exv4.attention_v4 = True
    V.check(exv4.encode(c["video"], layer=1), ref["feat"], **V.FP16_TOL)


# ---- the public interface -------------------------------------------------------------------------------------------------------------------
def test_public_interface(tmp_path, monkeypatch):
    c = V.make_case("main")
    video, sd, ref = c["video"], c["sd"], c["ref"][1]
    feats = get_dino_features_video(video, model_name="dinov2_vits14_reg", layer=1, state_dict=sd)
    assert feats.shape == (3, 384, 13, 17) and feats.device.type == "cpu"
    V.check(feats.permute(0, 2, 3, 1).reshape(3, 221, 384), ref["feat"], **V.FP16_TOL)
    keys = get_dino_features_video_packed(video, "dinov2_vits14_reg", facet="keys", layer=1, state_dict=sd)
    assert keys.shape == (3, 221, 384)
    V.check(keys, ref["qkv"][:, 5:, 384:768], **V.FP16_TOL)
    ex = _ex(c)
    shape = (3, 3, 98, 126)
    assert ex.get_patch_num(shape) == 226 and ex.get_height_patch_num(shape) == 13 and ex.get_width_patch_num(shape) == 17
    norm = (video - torch.tensor(A.IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.tensor(A.IMAGENET_STD).view(1, 3, 1, 1)
    k1 = ex.get_keys_from_input(norm, layers=[1])
    assert k1.shape == (3, 226, 384)
    V.check(k1, ref["qkv"][..., 384:768], **V.FP16_TOL)
    assert ex.get_feature_from_input(norm, layers=[1]).shape == (3, 226, 384)
    with pytest.raises(ValueError, match="register_tokens"):
        VitExtractor("dinov2_vits14", stride=7, device=DEV, state_dict=sd)
    with pytest.raises(KeyError, match="register_tokens"):
        VitExtractor("dinov2_vits14_reg", stride=7, device=DEV, state_dict=V.without_registers(sd))
    # an upstream-named register checkpoint: extra keys (mask_token, the final norm) are present and ignored, pos_embed is 1 x 1370 x D
    ckpt = dict(sd, mask_token=torch.zeros(1, 384), **{"norm.weight": torch.ones(384), "norm.bias": torch.zeros(384)})
    assert ckpt["pos_embed"].shape == (1, 1370, 384) and ckpt["register_tokens"].shape == (1, 4, 384)
    path = tmp_path / "dinov2_vits14_reg4_pretrain.pth"
    torch.save(ckpt, str(path))
    monkeypatch.setenv("DTK_DINOV2_WEIGHTS", str(path))
    from_file = VitExtractor("dinov2_vits14_reg", stride=7, device=DEV)
    assert from_file.n_registers == 4 and from_file.n_blocks == 2
    assert torch.equal(from_file.encode(video, layer=1), ex.encode(video, layer=1))
    # the name a preprocessing config carries reaches the extractor through get_dino_features_video (what save_dino_embed_video.py calls)
    config = {"dino_model_name": "dinov2_vits14_reg", "dino_stride": 7, "dino_layer": 1, "dino_facet": "tokens"}
    via = get_dino_features_video(video=video, model_name=config["dino_model_name"], facet=config["dino_facet"], stride=config["dino_stride"],
                                  layer=config["dino_layer"])
    assert torch.equal(via, feats)


def test_c_abi_refuses_bad_register_fields():
    """n_registers < 0, > 16, or a null `registers` with n_registers > 0: refused with a message before any device call (an untouched
    output buffer); a zero-initialised tail is the plain model (every existing positional construction of VitModel)."""
    import ctypes
    from dino_tracker_amd import _lib
    c = V.make_case("main")
    ex = _ex(c)
    frames = c["video"].to(DEV).contiguous()
    ex.encode(c["video"], layer=0)                       # builds the members the struct points to
    pos, cls_pos = ex._pos_embed(13, 17)

    def model(n_reg, regs):
        return _lib.VitModel(384, 6, 1, 14, 7, 1e-6, 0, ex._sd["patch_embed.proj.weight"].data_ptr(), ex._sd["patch_embed.proj.bias"].data_ptr(),
                             cls_pos.data_ptr(), pos.data_ptr(), ex._ms[True].data_ptr(),
                             ctypes.cast(ex._build_layers("fp16"), ctypes.POINTER(_lib.VitLayer)), 0, ex._overflow.data_ptr(), None, 0, 0.0, 0, 0,
                             n_reg, regs)

    ws = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    out = torch.full((3, 242, 384), 7.0, device=DEV)
    for n_reg, regs, what in ((-1, None, "n_registers"), (17, ex._sd["register_tokens"].data_ptr(), "n_registers"), (4, None, "null")):
        rc = _lib.lib().dtk_vit_forward(model(n_reg, regs), ops._p(frames), 3, 98, 126, ops._p(out), None, None, ops._p(ws), ws.numel(), ops._stream())
        assert rc != 0
        with pytest.raises(RuntimeError, match=what):
            _lib.check(rc)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())


# ---- downstream -----------------------------------------------------------------------------------------------------------------------------
def test_tracker_runs_on_register_model_features():
    """Everything behind the encoder takes the register model's features unchanged: Tracker.set_video(video, dino_features=<those features>)
    + ModelInference.infer on 16 grid queries, against the oracle's refine + infer on the SAME features (the identical-features tolerance)."""
    from gpu_util import make_inference
    from dino_tracker_amd.tracker import Tracker
    c = V.make_case("main")
    video, T, H, W, C = c["video"], 3, 98, 126, 384
    packed = get_dino_features_video_packed(video, "dinov2_vits14_reg", layer=1, state_dict=c["sd"])
    assert packed.shape == (T, 13 * 17, C)
    head, delta = synth.synth_head_weights(3), synth.synth_delta_dino_weights(C, seed=4)
    trk = Tracker(video=video.to(DEV), dino_features=torch.zeros_like(packed), dino_patch_size=14, stride=7, device=DEV, track_method=ops.TRACK_MFMA)
    trk.tracker_head.load_state_dict(head)
    trk.delta_dino.load_state_dict(delta)
    trk.to(DEV).eval()
    trk.delta_dino.conv_operands = "split"                  # fp32-grade refinement, as gpu_util.make_tracker sets for oracle comparisons
    trk.set_video(video.to(DEV), dino_features=packed)
    trk.cache_refined_embeddings()
    queries = torch.cat([synth.grid_queries(4, 3, H, W, 0, margin=20.0), synth.grid_queries(2, 2, H, W, 2, margin=20.0)])
    assert queries.shape[0] == 16
    traj, occ = make_inference(trk, H, W, T).infer(queries.cuda())
    chw = ops.unpack_features(packed, 13, 17).cpu()
    rt, ro = A.infer(A.refine_features(video, chw, delta), queries, head, H, W)
    err = float((traj.cpu() - rt).abs().max())
    print(f"tracker on dinov2_vits14_reg features: max |position - oracle| = {err:.2e} px, {int(occ.sum())} occluded flags")
    assert err < PX_TOL and torch.equal(occ.cpu(), ro)
