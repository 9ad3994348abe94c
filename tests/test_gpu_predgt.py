"""GPU: the BADJA counts (dtk_badja_counts), the prediction-against-ground-truth primitives (dtk_render_pred_gt_prims), the ring
kind of the rasteriser and visualize_trajectories_with_gt against the restatement of tests/predgt_ref.py, on the golden of
tests/golden/predgt.npz (the unmodified reference with a recording cv2) and on scenes of the restatement's own.

Bounds (docs/PARITY.md, "Prediction against ground truth"): the counts, the records and the pure-selection pixels are EQUAL; the
numeric blend is within FOUR times the float32-against-float64 difference of the restatement itself on the same inputs, rounded up to
two digits.  The differences are computed on the CPU by tests/test_predgt_reference.py::test_float32_against_float64, which also
checks the numbers below against them."""
import math
import os
import pickle

import numpy as np
import pytest
import torch

import predgt_ref as P
import viz_ref as R
from test_gpu_render import check_blend, dev, host_records

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predgt.npz")

# docs/PARITY.md "Prediction against ground truth": 4 x the measured float32-against-float64 differences of predgt_ref
GOLDEN_BLEND_BOUND = 3.6e-5  # blended values in [0, 1], golden scene (opaque primitives on integer coordinates)
NUMERIC_BLEND_BOUND = 2.2e-6 # blended values in [0, 1], the 300 random primitives of the four kinds


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD, allow_pickle=False))


def colors01(gold):
    return gold["colors_without_red"].astype(np.float64) / 255.0


# ---- 1. BADJA counts -------------------------------------------------------------------------------------------------------------
def device_counts(pred, gt, occ, seg, scale=(1.0, 1.0)):
    from dino_tracker_amd import tapvid
    args = (dev(pred), torch.from_numpy(np.ascontiguousarray(gt)), torch.from_numpy(np.ascontiguousarray(occ)), dev(seg), scale)
    a = tapvid.badja_counts(*args)
    b = tapvid.badja_counts(*args)
    assert a.dtype == torch.int64 and torch.equal(a, b)                          # two calls: equal bits
    return tuple(a.cpu().tolist())


@pytest.mark.parametrize("which", ["none", "854"])
def test_badja_counts_golden(gold, which):
    from dino_tracker_amd import tapvid
    pred, gt, occ = P.golden_badja(gold, which)
    h, w = int(gold["badja_h"]), int(gold["badja_w"])
    scale = (1.0, 1.0) if which == "none" else (w / 854, h / 476)
    want = P.badja_counts(pred, gt, occ, gold["badja_seg"], scale)
    assert device_counts(pred, gt, occ, gold["badja_seg"], scale) == want
    assert device_counts(pred, gt, occ, (gold["badja_seg"] > 0).astype(np.float32) * 0.25, scale) == want      # float masks
    # the public entry point, on the benchmark entry and the predictions per start frame (device tensors and numpy arrays)
    frames = [int(f) for f in gold["badja_frames"]]
    config = {"h": h, "w": w, "segmentations": gold["badja_seg"], "target_points": {f: gold[f"badja_gt_{f}"] for f in frames},
              "occluded": {f: gold[f"badja_occ_{f}"] for f in frames}}
    size = None if which == "none" else (854, 476)
    for results in ({f: dev(gold[f"badja_pred_{which}_{f}"]) for f in frames},
                    {f: (dev(gold[f"badja_pred_{which}_{f}"]), None) for f in frames},
                    {f: gold[f"badja_pred_{which}_{f}"] for f in frames}):
        m = tapvid.badja_metrics(results, config, size)
        assert m == P.badja_metrics(want)
        assert abs(m["acc_seg"] - gold[f"badja_acc_{which}"][0]) < 1e-3 and abs(m["acc_3px"] - gold[f"badja_acc_{which}"][1]) < 1e-3


def test_badja_counts_small_and_empty():
    from dino_tracker_amd import tapvid
    seg = np.zeros((2, 9, 11), dtype=np.uint8)
    seg[1, 2:7, 3:8] = 9                                                        # area 25: thr = 1
    gt = np.array([[[4.0, 4.0], [5.0, 5.0]]])
    for pred, want in (([[[0, 0], [5.5, 5.0]]], (1, 1, 1)), ([[[0, 0], [6.5, 5.0]]], (1, 0, 1)), ([[[0, 0], [5.0, 8.5]]], (1, 0, 0))):
        pred = np.array(pred, dtype=np.float32)
        assert device_counts(pred, gt, np.zeros((1, 2), dtype=np.uint8), seg) == want == P.badja_counts(pred, gt, np.zeros((1, 2)), seg)
    # nothing visible: zeros, and nan metrics without an exception
    pred = np.zeros((3, 2, 2), dtype=np.float32)
    counts = device_counts(pred, np.zeros((3, 2, 2)), np.ones((3, 2), dtype=bool), seg)
    assert counts == (0, 0, 0)
    m = tapvid.metrics_from_badja_counts(counts)
    assert math.isnan(m["acc_seg"]) and math.isnan(m["acc_3px"])
    config = {"h": 9, "w": 11, "segmentations": seg, "target_points": {0: np.zeros((3, 2, 2))}, "occluded": {0: np.ones((3, 2), dtype=bool)}}
    m = tapvid.badja_metrics({0: dev(pred)}, config, None)
    assert math.isnan(m["acc_seg"]) and math.isnan(m["acc_3px"])
    # frame 0 never counts, and T_seg = 1 scores nothing
    assert device_counts(pred, np.zeros((3, 2, 2)), np.zeros((3, 2), dtype=np.uint8), seg[:1]) == (0, 0, 0)


@pytest.mark.parametrize("masks", ["uint8", "float32"])
def test_badja_counts_random(masks):
    """2 000 points over several blocks, T_seg < T, distances at least 1e-6 (relative) away from every threshold."""
    pred, gt, occ, seg = P.random_badja()
    if masks == "float32":
        seg = np.where(seg > 0, np.float32(0.5), np.float32(-1.0))              # negative and zero are background
    want = P.badja_counts(pred, gt, occ, seg, (0.75, 1.25))
    assert device_counts(pred, gt, occ, seg, (0.75, 1.25)) == want
    assert want[0] > 5000 and 0 < want[1] < want[0] and 0 < want[2] < want[0]


def test_evaluate_scores_a_dataset_folder(tmp_path, gold, capsys):
    """python -m dino_tracker_amd.evaluate with its own device scorers on a two-video folder built from the golden: the BADJA rows
    are the reference's numbers, the TAP-Vid rows equal tapvid.tapvid_metrics on the same tensors, the average row is their mean."""
    import csv
    from dino_tracker_amd import evaluate as E, tapvid
    frames = [int(f) for f in gold["badja_frames"]]
    h, w = int(gold["badja_h"]), int(gold["badja_w"])
    videos = []
    for idx in (0, 5):
        videos.append({"video_idx": idx, "h": h, "w": w, "segmentations": gold["badja_seg"],
                       "target_points": {f: gold[f"badja_gt_{f}"] for f in frames},
                       "occluded": {f: gold[f"badja_occ_{f}"].astype(bool) for f in frames},
                       "query_points": {f: gold[f"badja_gt_{f}"][:, f] for f in frames}})
        for sub in ("trajectories", "occlusions"):
            os.makedirs(tmp_path / "data" / str(idx) / sub)
        for f in frames:
            pred = gold[f"badja_pred_854_{f}"] + np.float32(idx)                # video 5: every prediction moved by (5, 5)
            np.save(tmp_path / "data" / str(idx) / "trajectories" / f"trajectories_{f}.npy", pred)
            np.save(tmp_path / "data" / str(idx) / "occlusions" / f"occlusion_preds_{f}.npy", gold[f"badja_occ_{f}"].astype(bool))
    with open(tmp_path / "bench.pkl", "wb") as fh:
        pickle.dump({"videos": videos}, fh)
    base = ["--dataset-root-dir", str(tmp_path / "data"), "--benchmark-pickle-path", str(tmp_path / "bench.pkl")]
    E.eval_dataset(E.make_parser().parse_args(base + ["--out-file", str(tmp_path / "badja.csv"), "--dataset-type", "BADJA"]))
    rows = {r[0]: r[1:] for r in csv.reader(open(tmp_path / "badja.csv"))}
    assert rows["video_idx"] == ["acc_seg", "acc_3px"] and set(rows) == {"video_idx", "0", "5", "average"}
    assert all(abs(float(v) - ref) < 1e-3 for v, ref in zip(rows["0"], gold["badja_acc_854"]))
    assert float(rows["5"][0]) < float(rows["0"][0])
    assert [float(v) for v in rows["average"]] == [(float(a) + float(b)) / 2 for a, b in zip(rows["0"], rows["5"])]
    E.eval_dataset(E.make_parser().parse_args(base + ["--out-file", str(tmp_path / "tapvid.csv")]))
    rows = {r[0]: r[1:] for r in csv.reader(open(tmp_path / "tapvid.csv"))}
    results = {f: (dev(gold[f"badja_pred_854_{f}"]), dev(gold[f"badja_occ_{f}"].astype(bool))) for f in frames}
    want = tapvid.tapvid_metrics(results, videos[0], pred_size=(854, 476))
    assert rows["video_idx"] == list(want) and rows["video_idx"][0] == "occlusion_accuracy" and rows["video_idx"][-1] == "average_pts_within_thresh"
    assert [float(v) for v in rows["0"]] == list(want.values()) and float(rows["0"][0]) == 1.0
    assert capsys.readouterr().out.count("Total metrics:") == 2


# ---- 2. primitives ---------------------------------------------------------------------------------------------------------------
def test_pred_gt_prims_against_the_restatement(gold):
    """dtk_render_pred_gt_prims, every frame of the golden scene, one frame per call and all frames in one call: the inputs are
    integers, so every word is equal -- except 1 / |p1 - p0|^2, a float32 division, which is compared to one unit in the last
    place and is what it is in the restatement's float32 run."""
    from dino_tracker_amd import ops
    T = gold["scene_video"].shape[0]
    pxy, gxy = dev(P.int_points(gold["scene_pred"]), torch.int32), dev(P.int_points(gold["scene_gt"]), torch.int32)
    pocc, gocc = dev(gold["scene_pred_occ"] != 0, torch.uint8), dev(gold["scene_gt_occ"] != 0, torch.uint8)
    col = dev(colors01(gold), torch.float32)
    par = (int(gold["thickness"]), int(gold["radius"]), int(gold["cross_size"]))
    whole = host_records(ops.render_pred_gt_prims(pxy, gxy, pocc, gocc, col, 0, T, *par))
    n = pxy.shape[0]
    assert whole.shape == (2 * n * T, 12)
    want32 = P.golden_records(gold, colors01(gold), range(T), dtype=np.float32)
    kinds = set()
    for i in range(T):
        want = want32[i].astype(np.float64)
        got = host_records(ops.render_pred_gt_prims(pxy, gxy, pocc, gocc, col, i, 1, *par))
        assert got.shape == want.shape and (got[:, 11] == 0).all()
        np.testing.assert_array_equal(got[:, :10], want[:, :10])                # kind, geometry, size, colour, a
        seg = (want[:, 0] == P.SEGMENT) & (want[:, 9] > 0)
        np.testing.assert_array_equal(got[~seg, 10], want[~seg, 10])            # the ring's hw; 0 for discs and undrawn records
        assert (np.abs(got[seg, 10] - want[seg, 10]) <= np.spacing(want[seg, 10].astype(np.float32))).all()
        part = whole[2 * n * i:2 * n * (i + 1)]
        assert (part[:, 11] == i).all()
        np.testing.assert_array_equal(part[:, :11], got[:, :11])                # grouping changes the frame word only
        kinds |= {(int(r[0]), float(r[9])) for r in got}
    assert kinds == {(P.SEGMENT, 1.0), (P.SEGMENT, 0.0), (P.DISC, 1.0), (P.RING, 1.0)}


# ---- 3. ring binning -------------------------------------------------------------------------------------------------------------
def test_ring_binning():
    """Counts equal the tiles of the box grown by r + hw + 0.5; the keys name exactly those tiles."""
    from dino_tracker_amd import ops
    H, W = 50, 70
    rows = [P.ring_row(16, 16, 3, 1.0, (1, 0, 0)),        # straddles four tiles: box 11.5 .. 20.5
            P.ring_row(8, 8, 5, 1.0, (1, 0, 0)),          # box 1.5 .. 14.5: one tile
            P.ring_row(8, 8, 5, 2.0, (1, 0, 0)),          # box 0.5 .. 15.5, rounded outwards: the stroke width alone adds tiles
            P.ring_row(-2, 30, 6, 1.0, (1, 0, 0)),        # partly outside on the left
            P.ring_row(66, 47, 5, 0.5, (1, 0, 0)),        # across the ragged right / bottom corner
            P.ring_row(-30, -30, 8, 1.0, (1, 0, 0)),      # wholly outside: no key
            P.ring_row(35, 25, 40, 1.0, (1, 0, 0)),       # larger than the frame: every tile
            P.ring_row(35, 25, 4, 1.0, (1, 0, 0), a=0.0)]  # a = 0: no key
    rec = np.array(rows, dtype=np.float64)
    want = P.tile_counts(rec, H, W)
    np.testing.assert_array_equal(want, [4, 1, 4, 2, 4, 0, 20, 0])
    d = dev(R.device_records(rec))
    counts = ops.render_tile_counts(d, 1, H, W).cpu().numpy()
    np.testing.assert_array_equal(counts, want)
    ends = torch.cumsum(dev(counts), 0, dtype=torch.int64)
    K = int(ends[-1])
    keys = ops.render_tile_keys(d, (ends - dev(counts)).contiguous(), K, 1, H, W).cpu().numpy()
    assert len(np.unique(keys)) == K == want.sum()
    tile, p = keys >> 32, keys & 0xFFFFFFFF
    np.testing.assert_array_equal(np.bincount(p, minlength=len(rec)), want)
    assert sorted(tile[p == 0]) == [0, 1, 5, 6] and sorted(tile[p == 3]) == [5, 10] and sorted(tile[p == 4]) == [13, 14, 18, 19]


# ---- 4. exact picture ------------------------------------------------------------------------------------------------------------
def test_exact_picture_with_rings():
    """Opaque primitives on integer coordinates, rings among more than two LDS chunks of records in one tile: wherever the float64
    picture is a pure selection the output is BIT-EQUAL to the restatement."""
    from dino_tracker_amd import ops
    frames, rec = P.exact_scene()
    d = dev(R.device_records(rec))
    F, H, W = frames.shape[:3]
    counts = ops.render_tile_counts(d, F, H, W)
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    keys = ops.render_tile_keys(d, (ends - counts).contiguous(), int(ends[-1]), F, H, W).cpu().numpy()
    crowded = (keys >> 32) == 1 * 5 + 1
    in_tile = keys[crowded] & 0xFFFFFFFF
    assert crowded.sum() > 2 * ops.RENDER_CHUNK and (rec[in_tile, 0] == P.RING).sum() >= 40
    u8, f32 = ops.render_records(dev(frames), d, want_float=True)
    u8, f32 = u8.cpu().numpy(), f32.cpu().numpy()
    ref = P.blend(frames[0], rec)
    mask = P.exact_mask(frames.shape[1:3], rec)
    print(f"exact picture: {int(mask.sum())} of {mask.size} pixels compared bit for bit ({mask[16:32, 16:32].mean():.2f} of the "
          f"crowded tile); max |f32 - f64| anywhere {np.abs(f32[0] - ref).max():.3e}")
    assert mask.mean() > 0.8 and mask[16:32, 16:32].mean() > 0.25
    np.testing.assert_array_equal(u8[0][mask], R.to_u8(ref)[mask])
    np.testing.assert_array_equal(f32[0][mask], ref.astype(np.float32)[mask])
    np.testing.assert_array_equal(u8[1], frames[1])
    ring_px = P.coverage(np.array(P.ring_row(52, 20, 8, 1.0, (0, 0, 0)), dtype=np.float64), *np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)), np.float64) == 1
    assert ring_px.sum() > 40 and (u8[0][ring_px] == np.array([51, 204, 102])).all()            # the big ring is there


# ---- 5. numeric blend ------------------------------------------------------------------------------------------------------------
def test_numeric_blend_four_kinds():
    """300 random primitives of the four kinds with a in (0, 1) on 80 x 50, check_blend's rules."""
    from dino_tracker_amd import ops
    frame, rec = P.numeric_scene()
    assert {int(k) for k in rec[:, 0]} == {0, 1, 2, 3} and ((rec[:, 9] > 0) & (rec[:, 9] < 1)).all()
    u8, f32 = ops.render_records(dev(frame[None]), dev(R.device_records(rec)), want_float=True)
    check_blend(u8[0].cpu().numpy(), f32[0].cpu().numpy(), P.blend(frame, rec), NUMERIC_BLEND_BOUND, "numeric blend, four kinds")


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("badja", [False, True])
def test_end_to_end(gold, badja):
    from dino_tracker_amd import visualize as V
    video = gold["scene_video"]
    kept = list(gold["kept_badja"]) if badja else list(range(video.shape[0]))
    args = (gold["scene_pred"], gold["scene_gt"], gold["scene_pred_occ"], gold["scene_gt_occ"])
    kw = dict(thickness=int(gold["thickness"]), radius=int(gold["radius"]), cross_size=int(gold["cross_size"]), badja_vis_type=badja)
    np.random.seed(int(gold["scene_seed"]))
    stats = {}
    u8, f32 = V.visualize_trajectories_with_gt(video, *args, return_float=True, stats=stats, **kw)
    assert isinstance(u8, np.ndarray) and u8.dtype == np.uint8 and u8.shape == (len(kept),) + video.shape[1:]
    assert stats["groups"] == 1 and stats["prims"] == 2 * 8 * len(kept)
    recs = P.golden_records(gold, colors01(gold), kept)
    ref = np.stack([P.blend(video[i], r) for i, r in zip(kept, recs)])
    check_blend(u8, f32, ref, GOLDEN_BLEND_BOUND, f"pred vs gt, badja_vis_type={badja}")
    assert all((u8[k] != video[i]).any() for k, i in enumerate(kept))
    # device tensors in, device tensor out; independent of the frame groups and of the memory budget
    dv = dev(video)
    targs = (dev(gold["scene_pred"]), dev(gold["scene_gt"]), dev(gold["scene_pred_occ"]), dev(gold["scene_gt_occ"]))
    outs = []
    for extra in (dict(), dict(group_frames=1), dict(group_frames=4), dict(memory_budget=1)):
        np.random.seed(int(gold["scene_seed"]))
        stats = {}
        o = V.visualize_trajectories_with_gt(dv, *targs, stats=stats, **kw, **extra)
        assert isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.uint8
        outs.append(o)
        assert stats["groups"] == {1: len(kept), 4: 2}.get(extra.get("group_frames"), len(kept) if "memory_budget" in extra else 1)
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    np.testing.assert_array_equal(outs[0].cpu().numpy(), u8)


def test_cli_writes_the_named_video(tmp_path, capsys, gold):
    """python -m dino_tracker_amd.visualize pred-vs-gt on a synthetic data folder, run in this process through main()."""
    from PIL import Image
    from dino_tracker_amd import visualize as V
    root = str(tmp_path / "scene")
    video = gold["scene_video"]
    T, H, W = video.shape[:3]
    for sub in ("video", "trajectories", "occlusions"):
        os.makedirs(os.path.join(root, sub))
    for t, frame in enumerate(video):
        Image.fromarray(frame).save(os.path.join(root, "video", f"{t:05d}.png"))
    target = {0: gold["scene_gt"], 3: gold["scene_gt"][:5]}
    occluded = {0: gold["scene_gt_occ"].astype(bool), 3: gold["scene_gt_occ"][:5].astype(bool)}
    with open(os.path.join(root, "bench.pkl"), "wb") as fh:
        pickle.dump({"videos": [{"video_idx": 4, "h": H, "w": W, "target_points": target, "occluded": occluded}]}, fh)
    for f, n in ((0, 8), (3, 5)):
        np.save(os.path.join(root, "trajectories", f"trajectories_{f}.npy"), gold["scene_pred"][:n] * np.float32(2))   # at 2x
        np.save(os.path.join(root, "occlusions", f"occlusion_preds_{f}.npy"), gold["scene_pred_occ"][:n] != 0)
    base = ["pred-vs-gt", "--data-path", root, "--benchmark-pickle-path", os.path.join(root, "bench.pkl"), "--video-id", "4",
            "--infer-res-size", str(2 * H), str(2 * W), "--fps", "2"]
    np.random.seed(int(gold["scene_seed"]))
    written = V.main(base)
    said = capsys.readouterr().out
    assert len(written) == 2 and said.count("save_video:") == 2 and "Saved to" in said
    assert [os.path.basename(os.path.splitext(w)[0]) for w in written] == ["pred_vs_gt_frame_idx_0_fps_2", "pred_vs_gt_frame_idx_3_fps_2"]
    assert all(os.path.exists(w) for w in written)
    if os.path.isdir(written[0]):
        files = sorted(os.listdir(written[0]))
        assert len(files) == T
        frame0 = np.asarray(Image.open(os.path.join(written[0], files[0])))
        want = R.to_u8(P.blend(video[0], P.golden_records(gold, colors01(gold), [0])[0]))
        assert frame0.shape == (H, W, 3) and np.abs(frame0.astype(int) - want.astype(int)).max() <= 1
    written = V.main(base[:-1] + ["3", "--only-first-frame", "--use-gt-occ", "--badja-vis-type"])      # another fps: another name
    assert len(written) == 1 and "pred_vs_gt_frame_idx_0_fps_3" in written[0]
    if os.path.isdir(written[0]):
        assert len(os.listdir(written[0])) == len(gold["kept_badja"])


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(gold):
    from dino_tracker_amd import ops, tapvid, visualize as V
    video = gold["scene_video"]
    args = (gold["scene_pred"], gold["scene_gt"], gold["scene_pred_occ"], gold["scene_gt_occ"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.visualize_trajectories_with_gt(torch.from_numpy(video), *args)
    with pytest.raises(AssertionError, match="must be the same shape"):
        V.visualize_trajectories_with_gt(video, args[0], args[1][:5], args[2], args[3])
    with pytest.raises(RuntimeError, match="do not fit"):
        V.visualize_trajectories_with_gt(video, args[0], args[1], args[2][:, :4], args[3])
    pxy, gxy = dev(P.int_points(args[0]), torch.int32), dev(P.int_points(args[1]), torch.int32)
    pocc, gocc, col = dev(args[2] != 0, torch.uint8), dev(args[3] != 0, torch.uint8), dev(colors01(gold), torch.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_pred_gt_prims(pxy.cpu(), gxy, pocc, gocc, col, 0, 1)
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.render_pred_gt_prims(pxy, gxy[:, :3].contiguous(), pocc, gocc, col, 0, 1)
    with pytest.raises(RuntimeError, match="expected torch.int32"):
        ops.render_pred_gt_prims(pxy.float(), gxy, pocc, gocc, col, 0, 1)
    with pytest.raises(RuntimeError, match="bad sizes"):
        ops.render_pred_gt_prims(pxy, gxy, pocc, gocc, col, 4, 3)
    with pytest.raises(RuntimeError, match="thickness"):
        ops.render_pred_gt_prims(pxy, gxy, pocc, gocc, col, 0, 1, thickness=0)
    # dtk_render_prims still takes discs and diamonds only: the ring is not a marker of the track videos
    with pytest.raises(RuntimeError, match="marker_kind"):
        ops.render_prims(dev(args[0]), pocc, col, None, 0, 1, 50, 70, ops.RENDER_DOTTED, ops.RENDER_RING, 3.0)
    # BADJA: CPU predictions, shapes that do not fit, T_seg > T, a mask that could hold an area of 2^24
    pred, gt, occ = P.golden_badja(gold, "none")
    seg = gold["badja_seg"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tapvid.badja_counts(torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(occ), torch.from_numpy(seg))
    with pytest.raises(RuntimeError, match="do not fit"):
        tapvid.badja_counts(dev(pred), torch.from_numpy(gt[:3]), torch.from_numpy(occ), dev(seg))
    with pytest.raises(RuntimeError, match="T_seg"):
        tapvid.badja_counts(dev(pred), torch.from_numpy(gt), torch.from_numpy(occ), dev(np.zeros((pred.shape[1] + 1, 4, 4), dtype=np.uint8)))
    with pytest.raises(RuntimeError, match="2\\^24"):
        tapvid.badja_counts(dev(pred), torch.from_numpy(gt), torch.from_numpy(occ), torch.zeros((2, 4096, 4096), dtype=torch.uint8, device="cuda:0"))
