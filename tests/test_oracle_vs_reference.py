"""CPU: oracle restatements vs the UN-MODIFIED reference modules, through the reference's outputs on seeded inputs stored in
tests/golden/ref_units.npz (tests/golden/ref_units.py builds the inputs and, under make_golden.py, runs the reference)."""
import os

import numpy as np
import pytest
import torch

import ref_units as U
from oracle import ref_algo as A

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", U.GOLDEN)


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def test_delta_dino_and_align_match_reference(gold):
    c, sd, frames, vit = U.delta_dino_case()
    ref = torch.from_numpy(gold["delta_dino"])
    assert ref.shape == (2, c, 13, 17)
    cnn = A.delta_dino_cnn(frames, sd)
    assert cnn.shape[-2:] == (13, 16)  # 98->49->25->13, 126->63->32->16
    out = A.align_to_vit_grid(cnn, 13, 17)
    assert (out - ref).abs().max() < 1e-6


def test_tracker_forward_matches_reference(gold):
    H, W, T, video, feats, head, pts, tgt = U.tracker_forward_case()
    ref = torch.from_numpy(gold["tracker_forward"])
    src = A.sample_bilinear(feats, pts[:, :2], pts[:, 2], H, W)
    mine = A.track(src, feats, tgt, head, H, W)
    refpx = torch.stack([(ref[:, 0] + 1) / 2 * (W - 1), (ref[:, 1] + 1) / 2 * (H - 1)], 1)
    assert (mine - refpx).abs().max() < 1e-3


def test_vit_blocks_match_hf_port():
    """DINOv2 block arithmetic vs the independent transformers port (random weights mapped across).  Runs in a
    clean interpreter: the torchvision shim used for the reference must not be visible to transformers."""
    import os
    import subprocess
    import sys
    pytest.importorskip("transformers")
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hf_crosscheck.py")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


def test_tapvid_metrics_match_reference(gold):
    """oracle.tapvid_metrics vs the reference's compute_tapvid_metrics_for_video (eval/metrics.py:150-223) fed through
    its own .npy / pickle-dict interface, on random tracks with realistic error scales."""
    cfg, preds = U.tapvid_case()
    want = dict(zip(gold["tapvid_names"].tolist(), gold["tapvid_values"].tolist()))
    frames = list(cfg["query_points"])
    got = A.tapvid_metrics(np.concatenate([[f] * len(cfg["query_points"][f]) for f in frames]),
                           np.concatenate([cfg["occluded"][f] for f in frames]),
                           np.concatenate([cfg["target_points"][f] for f in frames]),
                           np.concatenate([preds[f][1] for f in frames]), np.concatenate([preds[f][0] for f in frames]),
                           (854, 476), (256, 256))
    assert set(got) == set(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], abs=1e-12), k
    assert 0.05 < want["average_jaccard"] < 0.95  # a non-degenerate case


def test_best_buddies_match_reference(gold):
    """oracle.best_buddies_pair vs the reference script preprocessing_dino_bb/extract_dino_best_buddies.py run as is (CPU)."""
    T, Hh, Ww, feats = U.best_buddies_case()
    C = feats.shape[1]
    bb = {k: {f: torch.from_numpy(gold[f"bb_{k}_{f}"]) for f in ("source_coords", "target_coords", "cos_sims")}
          for k in gold["bb_pairs"].tolist()}
    from dino_tracker_amd.best_buddies import create_meshgrid
    coords = create_meshgrid(Hh, Ww)
    tm = feats.permute(0, 2, 3, 1).reshape(T, -1, C)
    assert len(bb) == T * (T - 1)
    for s in range(T):
        for t in range(T):
            if s == t:
                continue
            si, ti, cs = A.best_buddies_pair(tm[s], tm[t])
            e = bb[f"{s}_{t}"]
            assert torch.equal(e["source_coords"].cpu(), coords[si]) and torch.equal(e["target_coords"].cpu(), coords[ti])
            assert (e["cos_sims"].cpu() - cs).abs().max() < 1e-6


def test_bb_nms_ratio_matches_reference_functions(gold):
    """N4 second half: oracle.bb_nms_ratio (no NMS sweep: arg-max + best non-overlapping candidate) vs the reference's
    get_bb_sim_indices / compute_bb_nms / compute_max_r (preprocessing_dino_bb/compute_dino_bb_nms.py:12-78) run as they
    are, around the restated torchvision.ops.batched_nms of oracle/shims (torchvision is absent: that one op is
    'parity unpinned').  Smooth random feature fields give rows with several separated peaks, so r takes values over (0, 1)."""
    T, ph, pw, feats, coords, tm, bbs = U.bb_nms_case()
    seen_r = []
    for (s, t) in U.BB_NMS_PAIRS:
        got = {}
        for a, b in ((s, t), (t, s)):
            e = bbs[f"{a}_{b}"]
            src = tm[a][(e["source_coords"][:, 1].long() - 7) // 7 * pw + (e["source_coords"][:, 0].long() - 7) // 7]
            aff = (src @ tm[b].t()) / torch.clamp(src.norm(dim=1)[:, None] * tm[b].norm(dim=1)[None], min=1e-8)
            top2, r = A.bb_nms_ratio(aff, pw, 50.0, 0.2, 400)
            got[(a, b)] = (top2, r)
            assert (torch.from_numpy(gold[f"nms_{a}_{b}_peak_affs"]) - top2).abs().max() < 1e-6
            assert (torch.from_numpy(gold[f"nms_{a}_{b}_r"]) - r).abs().max() < 1e-6
            seen_r.append(r)
        bb_r, bbr_r = torch.from_numpy(gold[f"max_r_{s}_{t}"]), torch.from_numpy(gold[f"max_r_{t}_{s}"])
        # compute_max_r by index arithmetic: pair i of (s, t) <-> the pair of (t, s) whose source is i's target
        cell = lambda xy: (xy[:, 1].long() - 7) // 7 * pw + (xy[:, 0].long() - 7) // 7  # noqa: E731
        where = torch.full((ph * pw,), -1, dtype=torch.long)
        where[cell(bbs[f"{t}_{s}"]["source_coords"])] = torch.arange(bbs[f"{t}_{s}"]["source_coords"].shape[0])
        j = where[cell(bbs[f"{s}_{t}"]["target_coords"])]
        m = torch.maximum(got[(s, t)][1], got[(t, s)][1][j])
        assert (bb_r - m).abs().max() < 1e-6
        rr = got[(t, s)][1].clone()
        rr[j] = m
        assert (bbr_r - rr).abs().max() < 1e-6
    allr = torch.cat(seen_r)
    assert allr.numel() > 50 and (allr > 0.05).float().mean() > 0.3 and (allr < 0.9).float().mean() > 0.3  # non-degenerate
