"""CPU: the restatement of tests/predgt_ref.py and the host half of the prediction-against-ground-truth video, the BADJA score and
the evaluation command against what the unmodified reference did (tests/golden/predgt.npz, make_golden_predgt.py: a recording cv2).

test_float32_against_float64 computes the float32-against-float64 differences of the restatement's blend on the inputs of
tests/test_gpu_predgt.py; four times those are the device bounds hard-coded there (docs/PARITY.md)."""
import argparse
import csv
import math
import os
import pickle

import numpy as np
import pytest

import predgt_ref as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predgt.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD, allow_pickle=False))


def colors01(gold):
    return gold["colors_without_red"].astype(np.float64) / 255.0


def test_get_colors_draws_what_the_reference_draws(gold):
    from dino_tracker_amd import visualize as V
    n, seed = len(gold["colors_plain"]), int(gold["scene_seed"])
    for key, without_red in (("colors_plain", False), ("colors_without_red", True)):
        np.random.seed(seed)
        got = V.get_colors(n, seed=0, without_red=without_red)
        assert all(isinstance(v, int) for c in got for v in c)
        np.testing.assert_array_equal(np.array(got), gold[key])
        np.testing.assert_array_equal(np.array(V.get_colors(n, 0, without_red, rng=np.random.RandomState(seed))), gold[key])
    np.random.seed(seed)
    assert V.get_colors(n, seed=1, without_red=True) != [tuple(c) for c in gold["colors_without_red"]]     # the shuffle's seed


@pytest.mark.parametrize("name", ["plain", "badja"])
def test_records_reproduce_the_recorded_draw_calls(gold, name):
    """Same primitives, same order, same integer geometry, same colours as the reference's cv2.line / cv2.circle calls."""
    kept = P.badja_frames(gold["scene_gt"]) if name == "badja" else list(range(gold["scene_video"].shape[0]))
    np.testing.assert_array_equal(kept, gold[f"kept_{name}"])
    recs = P.golden_records(gold, colors01(gold), kept)
    n = gold["scene_pred"].shape[0]
    assert all(r.shape == (2 * n, 12) for r in recs)
    calls = np.concatenate([P.calls_of(r, pos, int(i)) for pos, (r, i) in enumerate(zip(recs, kept))])
    np.testing.assert_array_equal(calls, gold[f"calls_{name}"])
    # the scene exercises truncation: floor would move these points
    assert (P.int_points(gold["scene_pred"]) != np.floor(gold["scene_pred"]).astype(int)).any()
    kinds = {int(r[0]) for rec in recs for r in rec if r[9] > 0}
    assert kinds == {P.SEGMENT, P.DISC, P.RING} and any((rec[:, 9] == 0).any() for rec in recs)


def test_frame_filter_and_package_helpers(gold):
    from dino_tracker_amd import visualize as V
    np.testing.assert_array_equal(V.badja_frames(gold["scene_gt"]), gold["kept_badja"])
    assert len(gold["kept_badja"]) < gold["scene_video"].shape[0]
    with pytest.raises(AssertionError, match="pred and gt trajectories must be the same shape"):
        V.visualize_trajectories_with_gt(gold["scene_video"], gold["scene_pred"], gold["scene_gt"][:, :3], None, None)


def test_ring_coverage():
    """clamp(0.5 + hw - |d - r|, 0, 1): 1 on the stroke, a one-pixel ramp on either side, 0 at the centre and far outside."""
    Y, X = np.meshgrid(np.arange(40.0), np.arange(40.0), indexing="ij")
    r = np.array(P.ring_row(20, 20, 8, 1.0, (1, 1, 1)), dtype=np.float64)
    cov = P.coverage(r, X, Y, np.float64)
    assert cov[20, 28] == 1 and cov[20, 12] == 1 and cov[28, 20] == 1          # d = r
    assert cov[20, 29] == 0.5 and cov[20, 27] == 0.5                            # |d - r| = 1 = hw: the middle of the ramp
    assert cov[20, 30] == 0 and cov[20, 26] == 0 and cov[20, 20] == 0           # |d - r| = 2 >= hw + 0.5
    d = np.hypot(X - 20, Y - 20)
    np.testing.assert_allclose(cov, np.clip(1.5 - np.abs(d - 8), 0, 1), atol=0)
    assert ((cov > 0) & (cov < 1)).any()
    assert P.grow(r[None])[0] == 9.5                                            # r + hw + 0.5


@pytest.mark.parametrize("which", ["none", "854"])
def test_badja_numbers(gold, which):
    """Counts exactly, acc_* within 1e-3 on the 0 .. 100 scale of the reference's float32 mean of flags."""
    pred, gt, occ = P.golden_badja(gold, which)
    h, w = int(gold["badja_h"]), int(gold["badja_w"])
    scale = (1.0, 1.0) if which == "none" else (w / 854, h / 476)
    counts = P.badja_counts(pred, gt, occ, gold["badja_seg"], scale)
    # the counts the reference's means imply, as integers
    want = gold[f"badja_acc_{which}"]
    assert counts[0] == int((occ[:, 1:gold["badja_seg"].shape[0]] == 0).sum()) and counts[0] > 0
    for got, ref in zip(counts[1:], want):
        assert got == int(round(ref * counts[0] / 100.0))
    m = P.badja_metrics(counts)
    assert abs(m["acc_seg"] - want[0]) < 1e-3 and abs(m["acc_3px"] - want[1]) < 1e-3
    assert 0 < counts[1] < counts[0] and 0 < counts[2] < counts[0] and counts[1] != counts[2]
    from dino_tracker_amd import tapvid
    assert tapvid.metrics_from_badja_counts(counts) == m
    nan = tapvid.metrics_from_badja_counts((0, 0, 0))
    assert math.isnan(nan["acc_seg"]) and math.isnan(nan["acc_3px"])


def float32_differences(gold):
    """{name: max |float32 run - float64 run| of the restatement's blend} on the inputs of the GPU tests."""
    video = gold["scene_video"]
    out = {"golden_blend": 0.0}
    for kept in (list(range(video.shape[0])), list(gold["kept_badja"])):
        r64 = P.golden_records(gold, colors01(gold), kept)
        r32 = P.golden_records(gold, colors01(gold), kept, dtype=np.float32)
        for i, a, b in zip(kept, r32, r64):
            np.testing.assert_array_equal(a[:, :6], b[:, :6])                  # integer geometry: the same in either precision
            out["golden_blend"] = max(out["golden_blend"], float(np.abs(P.blend(video[i], a, np.float32) - P.blend(video[i], b)).max()))
    frame, rec = P.numeric_scene()
    out["numeric_blend"] = float(np.abs(P.blend(frame, rec, np.float32) - P.blend(frame, rec)).max())
    return out


def test_float32_against_float64(gold):
    """The measured differences, printed; the device bounds of tests/test_gpu_predgt.py are FOUR times these (a different
    operation order and fused multiply-adds), rounded up to two digits -- checked here so the hard-coded numbers cannot drift."""
    import test_gpu_predgt as G
    d = float32_differences(gold)
    print("float32 against float64 (predgt_ref):", {k: f"{v:.3e}" for k, v in d.items()})
    for name, bound in (("golden_blend", G.GOLDEN_BLEND_BOUND), ("numeric_blend", G.NUMERIC_BLEND_BOUND)):
        assert 4 * d[name] <= bound <= 4 * d[name] * 1.05, (name, d[name], bound)


def test_exact_scene_is_mostly_a_pure_selection():
    """What the GPU test relies on, from the restatement alone: more than 0.8 of the pixels compare bit for bit, the crowded tile
    holds more than two chunks of records with rings among them and still has pure-selection pixels."""
    frames, rec = P.exact_scene()
    mask = P.exact_mask(frames.shape[1:3], rec)
    inside = (rec[:, 1] >= 16) & (rec[:, 1] < 32) & (rec[:, 2] >= 16) & (rec[:, 2] < 32)
    print(f"exact scene: {mask.mean():.3f} of the pixels are pure selections, {mask[16:32, 16:32].mean():.3f} of the crowded tile; "
          f"{int(inside.sum())} records start in it, {int((inside & (rec[:, 0] == P.RING)).sum())} of them rings")
    assert mask.mean() > 0.8 and mask[16:32, 16:32].mean() > 0.25
    assert inside.sum() > 2 * 256 and (inside & (rec[:, 0] == P.RING)).sum() >= 40


# ---- the evaluation command, with the metric functions injected ----------------------------------------------------------------------
def write_dataset(root):
    for idx in ("0", "7"):
        os.makedirs(os.path.join(root, "data", idx, "trajectories"))
        os.makedirs(os.path.join(root, "data", idx, "occlusions"))
    os.makedirs(os.path.join(root, "data", ".cache"))                            # skipped: starts with a dot
    bench = {"videos": [{"video_idx": 0, "h": 48, "w": 64}, {"video_idx": 7, "h": 48, "w": 64}]}
    with open(os.path.join(root, "bench.pkl"), "wb") as fh:
        pickle.dump(bench, fh)
    return argparse.Namespace(dataset_root_dir=os.path.join(root, "data"), benchmark_pickle_path=os.path.join(root, "bench.pkl"),
                              out_file=os.path.join(root, "out", "metrics.csv"), dataset_type="BADJA", pred_video_sizes=(854, 476))


def test_evaluate_writes_the_reference_csv(tmp_path, capsys):
    from dino_tracker_amd import evaluate as E
    args = write_dataset(str(tmp_path))
    seen = []

    def badja_fn(trajectories_dir, config, sizes):
        seen.append((os.path.basename(os.path.dirname(trajectories_dir)), config["video_idx"], list(sizes)))
        if config["video_idx"] == 0:
            return {"acc_seg": 40.0, "acc_3px": float("nan"), "only_nan": float("nan")}
        return {"acc_seg": 60.5, "acc_3px": 30.25, "only_nan": float("nan")}

    means = E.eval_dataset(args, badja_fn=badja_fn)
    assert sorted(seen) == [("0", 0, [854, 476]), ("7", 7, [854, 476])]
    rows = list(csv.reader(open(args.out_file)))
    assert rows[0] == ["video_idx", "acc_seg", "acc_3px", "only_nan"]          # the metric dict's order
    by = {r[0]: r[1:] for r in rows[1:]}
    assert rows[-1][0] == "average" and set(by) == {"0", "7", "average"} and len(rows) == 4
    assert by["0"] == ["40.0", "", ""] and by["7"] == ["60.5", "30.25", ""]
    assert by["average"] == ["50.25", "30.25", ""]                              # NaNs are skipped; a column of NaNs stays NaN
    assert means["acc_seg"] == 50.25 and means["acc_3px"] == 30.25 and math.isnan(means["only_nan"])
    assert "Total metrics:" in capsys.readouterr().out

    args.dataset_type = "tapvid"
    order = ["occlusion_accuracy", "pts_within_1", "jaccard_1", "average_jaccard", "average_pts_within_thresh"]
    E.eval_dataset(args, tapvid_fn=lambda tdir, odir, config, sizes: {k: float(config["video_idx"]) for k in order})
    rows = list(csv.reader(open(args.out_file)))
    assert rows[0] == ["video_idx"] + order and rows[-1] == ["average"] + ["3.5"] * 5
    args.dataset_type = "davis"
    with pytest.raises(ValueError, match="Invalid dataset type"):
        E.eval_dataset(args)


def test_evaluate_reports_a_missing_file_like_the_reference(tmp_path):
    """The default scorers fail on the first missing .npy with the reference's assertion text, before anything is uploaded."""
    from dino_tracker_amd import evaluate as E
    tdir, odir = str(tmp_path / "trajectories"), str(tmp_path / "occlusions")
    config = {"video_idx": 0, "h": 48, "w": 64, "target_points": {3: None}, "query_points": {3: None}}
    with pytest.raises(AssertionError, match="failed to load .*trajectories_3.npy"):
        E.badja_video_metrics(tdir, config, [854, 476], device="cpu")
    with pytest.raises(AssertionError, match="failed to load .*trajectories_3.npy"):
        E.tapvid_video_metrics(tdir, odir, config, [854, 476], device="cpu")
    os.makedirs(tdir)
    np.save(os.path.join(tdir, "trajectories_3.npy"), np.zeros((1, 2, 2), dtype=np.float32))
    with pytest.raises(AssertionError, match="failed to load .*occlusion_preds_3.npy"):
        E.tapvid_video_metrics(tdir, odir, config, [854, 476], device="cpu")
    parser = E.make_parser()
    assert tuple(parser.parse_args([]).pred_video_sizes) == (854, 476)
    assert parser.parse_args(["--dataset-type", "BADJA", "--pred-video-sizes", "64", "48"]).pred_video_sizes == [64, 48]
