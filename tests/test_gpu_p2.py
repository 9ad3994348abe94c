"""-m gpu: Delta-DINO refinement (P2) through the C-ABI vs the reference golden and the oracle.
Feature-level tolerance: 3e-5 abs on O(1) features (fp32 everywhere; only the summation order differs)."""
import os

import numpy as np
import pytest
import torch

import make_golden as MG
from dino_tracker_amd import ops, synth
from oracle import ref_algo as A

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FEAT_TOL = 3e-5


def test_refine_matches_reference_golden_and_tracks():
    from gpu_util import make_inference, make_tracker
    cfg = MG.CASES["p23_small"]
    gold = np.load(os.path.join(GOLD, "p23_small.npz"))
    video, dino, head, queries, delta = MG.build_inputs(cfg)
    trk = make_tracker(video, dino, head, delta=delta, method=ops.TRACK_MFMA)
    trk.eval()
    mi = make_inference(trk, cfg["H"], cfg["W"], cfg["T"])  # runs cache_refined_embeddings() on the HIP path
    refined = trk.refined_features.cpu().numpy()
    assert refined.shape == gold["refined"].shape
    assert np.abs(refined - gold["refined"]).max() < FEAT_TOL
    assert np.abs(refined - dino.numpy()).mean() > 0.01  # the residual is not trivially zero
    traj, occ = mi.infer(queries.cuda())
    assert np.abs(traj.cpu().numpy() - gold["traj"]).max() < 1e-3
    assert np.array_equal(occ.cpu().numpy(), gold["occ"])
    # arbitrary frame subset API (Tracker.get_refined_embeddings)
    sub = torch.tensor([3, 0])
    r, res = trk.get_refined_embeddings(sub)
    assert np.abs(r.cpu().numpy() - gold["refined"][[3, 0]]).max() < FEAT_TOL
    assert np.abs((r - res).cpu().numpy() - dino.numpy()[[3, 0]]).max() < 1e-6
    # the library's DEFAULT operand mode (plain fp16 conv operands since round 4) against the same reference-written golden, with
    # its own tolerance: refined features within 2e-3 of the residual's size, positions within 1e-3 px, flags equal
    trk_d = make_tracker(video, dino, head, delta=delta, method=ops.TRACK_MFMA, p2_operands=None)
    trk_d.eval()
    mi_d = make_inference(trk_d, cfg["H"], cfg["W"], cfg["T"])
    refined_d = trk_d.refined_features.cpu().numpy()
    res_scale = float(np.abs(gold["refined"] - dino.numpy()).max())
    err_d = float(np.abs(refined_d - gold["refined"]).max())
    traj_d, occ_d = mi_d.infer(queries.cuda())
    dpx = float(np.abs(traj_d.cpu().numpy() - gold["traj"]).max())
    print(f"default (fp16-operand) Delta-DINO vs the reference golden: refined err {err_d:.3g} ({err_d / res_scale:.2g} of the residual), "
          f"positions {dpx:.3g} px")
    assert err_d < 2e-3 * res_scale and dpx < 1e-3
    assert np.array_equal(occ_d.cpu().numpy(), gold["occ"])


@pytest.mark.parametrize("C,H,W", [(384, 476, 854), (32, 98, 126)])
def test_refine_fp16_operands_vs_oracle(C, H, W):
    """The library default since round 4: plain fp16 operands in the 5x5 convolutions of layers 2-4 (DTK_DD_FP16), fp32
    accumulation.  Four stages of 2^-11 operand rounding: the residual is within 2e-3 of its own size of the fp32 oracle's
    (measured 3-6e-4), and measurably different from the split mode (so the switch is live)."""
    from gpu_util import make_tracker
    T = 2
    ph, pw = A.feature_grid(H, W)
    video = synth.synth_video(T, H, W, seed=61)
    dino = synth.synth_features(T, C, ph, pw, seed=62)
    delta = synth.synth_delta_dino_weights(C, seed=63)
    ref = A.refine_features(video, dino, delta)
    res_scale = float((ref - dino).abs().max())
    got = {}
    for mode in ("fp16", "split", None):
        trk = make_tracker(video, dino, synth.synth_head_weights(3), delta=delta, p2_operands=mode)
        trk.eval()
        trk.cache_refined_embeddings()
        got[mode] = trk.refined_features.cpu()
    err16, err_split = float((got["fp16"] - ref).abs().max()), float((got["split"] - ref).abs().max())
    print(f"C={C}: residual scale {res_scale:.3g}, fp16-operand error {err16:.3g} ({err16 / res_scale:.2g} of the residual), split {err_split:.3g}")
    assert err16 < 2e-3 * res_scale
    assert err_split < FEAT_TOL and err16 > 2 * err_split
    if not os.environ.get("DTK_P2_OPERANDS"):
        assert torch.equal(got[None], got["fp16"]), "fp16 operands are the default"


@pytest.mark.parametrize("C,H,W", [(384, 476, 854), (32, 98, 126)])
def test_refine_vs_oracle(C, H, W):
    from gpu_util import make_tracker
    T = 2
    ph, pw = A.feature_grid(H, W)
    video = synth.synth_video(T, H, W, seed=61)
    dino = synth.synth_features(T, C, ph, pw, seed=62)
    delta = synth.synth_delta_dino_weights(C, seed=63)
    ref = A.refine_features(video, dino, delta)
    trk = make_tracker(video, dino, synth.synth_head_weights(3), delta=delta)
    trk.eval()
    trk.cache_refined_embeddings()
    got = trk.refined_features.cpu()
    assert (got - ref).abs().max() < FEAT_TOL
    feat, norms, _ = trk.features()
    assert (norms.cpu() - ref.norm(dim=1).reshape(T, -1)).abs().max() < 1e-4


@pytest.mark.parametrize("C,H,W", [(32, 99, 127), (32, 101, 131), (32, 143, 211), (32, 57, 71), (32, 119, 245), (384, 101, 131)])
def test_refine_odd_sizes_vs_oracle(C, H, W):
    """Frame sizes that are odd in both dimensions and, but for 119 x 245, no multiple of 7 (every other size of this file is even
    and, apart from 476, a multiple of 7): odd extents through the three BlurPools (99 -> 50 -> 25 -> 13), (H - 14) // 7 flooring in
    the token grid, and the alignment of a CNN map whose last cell lies short of the frame edge.  Split mode within FEAT_TOL, fp16 operands within 2e-3
    of the residual's size, norms within 1e-4 -- the bounds of the two tests above."""
    from gpu_util import make_tracker
    T = 2
    ph, pw = A.feature_grid(H, W)
    assert H % 2 == 1 and W % 2 == 1
    video = synth.synth_video(T, H, W, seed=61)
    dino = synth.synth_features(T, C, ph, pw, seed=62)
    delta = synth.synth_delta_dino_weights(C, seed=63)
    ref = A.refine_features(video, dino, delta)
    res_scale = float((ref - dino).abs().max())
    got = {}
    for mode in ("split", "fp16"):
        trk = make_tracker(video, dino, synth.synth_head_weights(3), delta=delta, p2_operands=mode)
        trk.eval()
        trk.cache_refined_embeddings()
        got[mode] = trk.refined_features.cpu()
        if mode == "split":
            _, norms, _ = trk.features()
            nerr = float((norms.cpu() - ref.norm(dim=1).reshape(T, -1)).abs().max())
    err_split, err16 = float((got["split"] - ref).abs().max()), float((got["fp16"] - ref).abs().max())
    print(f"C={C} {H}x{W} ({ph}x{pw}): residual scale {res_scale:.3g}, split {err_split:.3g}, fp16 operands {err16:.3g} "
          f"({err16 / res_scale:.2g} of the residual), norms {nerr:.3g}")
    assert got["split"].shape == ref.shape and torch.isfinite(got["split"]).all() and torch.isfinite(got["fp16"]).all()
    assert err_split < FEAT_TOL
    assert err16 < 2e-3 * res_scale
    assert nerr < 1e-4


def test_training_mode_is_refused():
    from gpu_util import make_tracker
    cfg = MG.CASES["p23_small"]
    video, dino, head, queries, delta = MG.build_inputs(cfg)
    trk = make_tracker(video, dino, head, delta=delta)
    trk.train()
    with pytest.raises(RuntimeError, match="eval-mode"):
        trk.cache_refined_embeddings()
