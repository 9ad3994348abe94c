"""-m gpu: dinov2_vitg14 (D = 1536, 24 heads, SwiGLU feed-forward) through the encoder and the public interface, against the float64
restatement of tests/vitg_ref.py.  Weights: the first two of the 40 blocks (synth.make_vit_weights(..., nblocks=2), LayerScale 1.0).
Frames: 3 x 98 x 126 -> 13 x 17 patch tokens, S = 222, 666 rows -- the 256-row tiles are ragged and frame ends fall inside tiles.
The float64 reference (and its float32 run, the yardstick of the split path) is computed once per module on the CPU.

Tolerances are the project's own: LayerScale-1.0 class of tests/test_gpu_p1.py (cos >= 0.999999, rel <= 8e-4), its bf16 class
(cos >= 0.999, rel <= 2e-2); split operands: relative Frobenius error <= 4 x that of the float32 restatement (docs/PARITY.md, the RAFT
rule).  The figures each test prints are recorded in docs/PARITY.md ("ViT-g/14")."""
import pytest
import torch

import vitg_ref as G
from dino_tracker_amd import ops, synth
from dino_tracker_amd.extractor import VitExtractor
from dino_tracker_amd.utils import get_dino_features_video
from oracle import ref_algo as A

pytestmark = pytest.mark.gpu

NAME = "dinov2_vitg14"
FP16_TOL = dict(cos_min=0.999999, rel_max=8e-4)
BF16_TOL = dict(cos_min=0.999, rel_max=2e-2)
PX_TOL = 1e-3       # tests/test_gpu_p3.py, the dense-anchor case


def _check(got, ref, cos_min, rel_max):
    got, ref = got.double().cpu(), ref.double()
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
    rel = (got - ref).norm() / ref.norm()
    assert cos.min() >= cos_min, (cos.min().item(), rel.item())
    assert rel <= rel_max, (cos.min().item(), rel.item())
    return cos.min().item(), rel.item()


def _rel(got, ref):
    return float((got.double().cpu() - ref.double()).norm() / ref.double().norm())


@pytest.fixture(scope="module")
def case():
    sd = synth.make_vit_weights(NAME, seed=9, nblocks=2)
    video = synth.synth_video(3, 98, 126, seed=73)
    sd64 = G.to64(sd)
    with torch.no_grad():
        ref = {l: G.vitg_tokens(video.double(), sd64, l, return_qkv=True) for l in (0, 1)}
        ref32 = G.vitg_tokens(video, sd, 1)
    return {"sd": sd, "video": video, "tok": {l: ref[l][0] for l in ref}, "qkv": {l: ref[l][1] for l in ref}, "tok32": ref32}


def _ex(case, **kw):
    return VitExtractor(NAME, stride=7, device="cuda:0", state_dict=case["sd"], **kw)


def test_encode_fast_fp16_and_bf16(case):
    ex = _ex(case)
    assert ex.cfg["depth"] == 40 and ex.get_n_layers() == 40 and ex.n_blocks == 2 and ex.get_head_num() == 24
    feat = ex.encode(case["video"], layer=1)
    assert feat.shape == (3, 13 * 17, 1536)
    # (measured: rel 7.99e-4, min cos 0.9999996 -- this width sits AT the LayerScale-1.0 tolerance after two blocks; one block is 6.6e-4.
    #  The kernels are deterministic, so the figure repeats; the stage tests bound every GEMM of the block far below its own limit.)
    cos, rel = _check(feat, case["tok"][1][:, 1:], **FP16_TOL)
    print(f"vitg fast fp16 block 1: min token cos {cos:.7f}, rel {rel:.2e}")
    exb = _ex(case, operand_dtype="bf16")
    cos, rel = _check(exb.encode(case["video"], layer=1), case["tok"][1][:, 1:], **BF16_TOL)
    print(f"vitg fast bf16 block 1: min token cos {cos:.7f}, rel {rel:.2e}")
    with pytest.raises(ValueError, match="state dict holds blocks"):
        ex.encode(case["video"], layer=2)


def test_encode_split_is_fp32_grade(case):
    ref = case["tok"][1]
    rel32 = _rel(case["tok32"], ref)
    ex = _ex(case, precision="split")
    tok = ex.encode(case["video"], layer=1, want="tokens")
    rel = _rel(tok, ref)
    print(f"vitg split fp16 block 1: rel {rel:.2e} (float32 restatement on the CPU: {rel32:.2e})")
    assert rel <= 4 * rel32, (rel, rel32)
    assert ex.precision_report()["split_blocks"] == list(range(40))


def test_tiled_gemms_match_the_wide_path(case):
    """One block on DTK_VIT_TILED_GEMMS against the LDS-DMA kernels: the same 16-bit operands, so they agree far more closely than
    either agrees with float64 -- and not bit for bit, so two kernels did run."""
    ex = _ex(case)
    a = ex.encode(case["video"], layer=0).cpu()
    ex.tiled_gemms = True
    b = ex.encode(case["video"], layer=0).cpu()
    print(f"vitg wide vs tiled GEMMs, block 0: rel {_rel(a, b):.2e}, bit-equal {torch.equal(a, b)}")
    assert not torch.equal(a, b)
    _check(a, b, cos_min=0.999999, rel_max=3e-4)
    exs = _ex(case, precision="split")
    a = exs.encode(case["video"], layer=0).cpu()
    exs.tiled_gemms = True
    b = exs.encode(case["video"], layer=0).cpu()
    print(f"vitg split-DMA vs split-tiled GEMMs, block 0: rel {_rel(a, b):.2e}, bit-equal {torch.equal(a, b)}")
    _check(a, b, cos_min=0.999999, rel_max=3e-4)


@pytest.mark.parametrize("precision", ["fast", "split"])
def test_layernorm_covers_all_1536_columns(case, precision):
    """The LayerNorm kernels hold six float4 of a row per lane at this width.  With four (the kernels before ViT-g) the columns
    1024 .. 1535 were neither summed nor written: the block output's error there must be what it is in the columns below."""
    tok = _ex(case, precision=precision).encode(case["video"], layer=0, want="tokens")
    ref = case["tok"][0]
    lo, hi = _rel(tok[..., :1024], ref[..., :1024]), _rel(tok[..., 1024:], ref[..., 1024:])
    print(f"vitg {precision} block 0: rel error channels 0..1023 {lo:.2e}, 1024..1535 {hi:.2e}")
    assert 0.5 <= hi / lo <= 2.0, (lo, hi)


def test_public_interface(case):
    video, sd = case["video"], case["sd"]
    feats = get_dino_features_video(video, model_name=NAME, layer=1, state_dict=sd)
    assert feats.shape == (3, 1536, 13, 17) and feats.device.type == "cpu"
    _check(feats.permute(0, 2, 3, 1).reshape(3, 221, 1536), case["tok"][1][:, 1:], **FP16_TOL)
    ex = _ex(case)
    norm = (video - torch.tensor(A.IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.tensor(A.IMAGENET_STD).view(1, 3, 1, 1)
    both = ex.get_feature_from_input(norm, layers=[0, 1])
    singles = torch.stack([ex.get_feature_from_input(norm, layers=[l]) for l in (0, 1)]).mean(dim=0)
    assert both.shape == (3, 222, 1536)
    rel = _rel(both, singles.cpu())
    print(f"vitg taps [0, 1] vs the mean of the single-layer calls: rel {rel:.2e}")
    assert rel <= 2e-6
    _check(both, (case["tok"][0] + case["tok"][1]) / 2, **FP16_TOL)
    qkv = ex.get_qkv_feature_from_input(norm)
    assert len(qkv) == 40
    assert qkv[1].shape == (3, 222, 4608)        # [B, 1 + 13 * 17, 3 D]
    _check(qkv[1], case["qkv"][1], cos_min=0.99999, rel_max=1e-3)
    assert ex.get_keys_from_input(norm, layers=[1]).shape == (3, 222, 1536)


def test_saved_embeddings_and_measured_precision(case, tmp_path):
    """save_dino_embed_video writes what get_dino_features_video returned; precision="auto-blocks" calibrates at depth 40 with the two
    blocks the state dict holds: the fast pass is beyond auto_tol at LayerScale 1.0, so blocks are escalated and the result is fp32-grade
    or within the fast tolerance, as the calibration says."""
    from dino_tracker_amd.utils import save_dino_embed_video
    video, sd = case["video"], case["sd"]
    feats = get_dino_features_video(video, model_name=NAME, layer=1, state_dict=sd)
    path = str(tmp_path / "dino_embeddings" / "dino_embed_video.pt")
    save_dino_embed_video(path, feats)
    back = torch.load(path)
    assert back.shape == (3, 1536, 13, 17) and torch.equal(back, feats)
    ex = _ex(case, precision="auto-blocks")
    tok = ex.encode(video, layer=1, want="tokens")
    cal = ex.calibration
    assert cal is not None and cal["layer"] == 1 and cal["chosen"] in ("fast", "blocks", "split")
    rep = ex.precision_report()
    print(f"vitg auto-blocks: fast-vs-split {cal['rel_fast_vs_split']:.2e}, chosen {cal['chosen']}, split blocks {rep['split_blocks'][:4]}...")
    assert cal["rel_fast_vs_split"] > cal["tol"] and cal["chosen"] != "fast"      # 8e-4 against auto_tol 2.5e-4
    _check(tok, case["tok"][1], **FP16_TOL)


def test_hidden_overflow_is_reported_and_healed(case):
    """The value half of ONE hidden unit of block 0 scaled by 2e5: silu(gate) * value leaves the fp16 range in many tokens (bit 4); the
    unit's w3 column is zero, so the residual update stays in range.  The default fallback re-encodes on split bf16 operands."""
    sd = {k: v.clone() for k, v in case["sd"].items()}
    H = G.HIDDEN
    sd["blocks.0.mlp.w12.weight"][H + 5] *= 2e5
    sd["blocks.0.mlp.w12.bias"][H + 5] *= 2e5
    sd["blocks.0.mlp.w3.weight"][:, 5] = 0.0
    assert float(sd["blocks.0.mlp.w12.weight"][H + 5].abs().max()) < 6.0e4
    video = case["video"]
    for tiled in (False, True):
        ex = VitExtractor(NAME, stride=7, device="cuda:0", state_dict=sd, on_overflow="raise")
        ex.tiled_gemms = tiled
        with pytest.raises(RuntimeError, match="fp16 range"):
            ex.encode(video, layer=1)
        assert ex.last_overflow & 4, ex.last_overflow
    exs = VitExtractor(NAME, stride=7, device="cuda:0", state_dict=sd, on_overflow="raise", precision="split")
    with pytest.raises(RuntimeError, match="fp16 range"):
        exs.encode(video, layer=1)
    assert exs.last_overflow & 4, exs.last_overflow
    exh = VitExtractor(NAME, stride=7, device="cuda:0", state_dict=sd)
    with pytest.warns(RuntimeWarning):
        healed = exh.encode(video, layer=1)
    assert exh.range_fallbacks == 1 and exh.operand_dtype == "bf16" and len(exh.split_blocks) == 40
    assert bool(torch.isfinite(healed).all())
    with torch.no_grad():
        ref = G.vitg_tokens(video[:1].double(), G.to64(sd), 1)[:, 1:]
    rel = _rel(healed[:1], ref)
    print(f"vitg planted hidden overflow, healed on split bf16: rel {rel:.2e}")
    assert rel <= BF16_TOL["rel_max"]


@pytest.mark.parametrize("method", [ops.TRACK_EXACT, ops.TRACK_MFMA], ids=["exact", "mfma"])
def test_tracker_inference_at_1536_channels(method):
    """Tracker / ModelInference on 1536-channel features take the generic kernels (no tracker kernel is specialised for this width):
    positions, cosine similarities and occlusion flags against the oracle at the tolerances of tests/test_gpu_p3.py's dense-anchor case."""
    from gpu_util import make_inference, make_tracker
    H, W, T, C = 98, 126, 4, 1536
    feats = synth.synth_features(T, C, 13, 17, seed=43)
    head = synth.synth_head_weights(3)
    queries = torch.cat([synth.grid_queries(4, 3, H, W, 0, margin=20.0), synth.grid_queries(2, 2, H, W, 2, margin=20.0)])
    assert queries.shape[0] == 16
    trk = make_tracker(torch.zeros(T, 3, H, W), feats, head, method=method)
    mi = make_inference(trk, H, W, T)
    traj, occ = mi.infer(queries.cuda())
    rt, ro, rcs, _ = A.infer(feats, queries, head, H, W, return_aux=True)
    err = float((traj.cpu() - rt).abs().max())
    print(f"vitg-width tracker, method {method}: max |position - oracle| = {err:.2e} px")
    assert err < PX_TOL
    cs = mi.compute_trajectory_cos_sims(mi.compute_trajectories(queries.cuda()), queries.cuda()).cpu()
    assert (cs - rcs).abs().max() < 1e-5
    assert torch.equal(occ.cpu(), ro)
