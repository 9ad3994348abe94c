"""Writes tests/golden/predgt.npz by running the UN-MODIFIED reference (needs a reference checkout, oracle/ref_harness.py
REFERENCE_ROOT):
    python tests/golden/make_golden_predgt.py

  (a) eval/metrics.py compute_badja_metrics_for_video on a synthetic benchmark entry and a folder of trajectories_<f>.npy,
      with pred_video_sizes None and [854, 476];
  (b) visualization/visualize_pred_vs_gt.py visualize_trajectories_with_gt on a 70 x 50 scene, with and without badja_vis_type,
      and visualization/viz_utils.py get_colors under a seeded np.random.

The reference draws with cv2, which is not installed: this generator puts a RECORDING `cv2` into sys.modules whose line / circle
draw nothing and note their arguments (oracle/shims is not used).  `tqdm` is replaced by a stand-in that notes which frame the
reference is on, and `data.data_utils` / `utils` (imageio, matplotlib, einops ...; only load_video, save_video and add_config_paths
are taken from them, and nothing run here calls those) by empty stand-ins.  What is recorded is the reference's primitives, their
order, integer geometry and colours.

Stored (data only, loadable with allow_pickle=False):
  scene_video [T, H, W, 3] uint8, scene_pred [N, T, 2] float32, scene_gt [N, T, 2] float64, scene_pred_occ / scene_gt_occ [N, T],
  scene_seed (np.random.seed before every reference call that draws colours), thickness / radius / cross_size,
  calls_plain / calls_badja [n_calls, 12] int64: position of the frame in the output, kind (0 line, 1 circle), x0, y0, x1, y1
      (circle: the centre twice), radius (lines: 0), thickness, r, g, b, and the source frame index,
  kept_plain / kept_badja: the frame indices the reference rendered,
  colors_plain / colors_without_red [N, 3]: get_colors(N, seed=0, without_red=False / True) after np.random.seed(scene_seed),
  badja_frames (target_points' keys, in the dict's order), badja_gt_<f> float64, badja_occ_<f>, badja_pred_none_<f> /
  badja_pred_854_<f> float32 (the same predictions in the benchmark raster and in 854 x 476), badja_seg [T_seg, h, w] uint8,
  badja_h / badja_w, badja_acc_none / badja_acc_854 = (acc_seg, acc_3px).

Asserted here: every BADJA distance is at least 1e-3 away from 3.0 and from its frame's threshold, and there is one within 0.05 on
either side of each; the scene has all four occlusion cases in frame 0, a point outside the frame, negative coordinates that
truncation and floor treat differently, a pred = gt point, and a frame the BADJA filter drops.
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402

OUT = os.path.join(HERE, "predgt.npz")
LOG = {"calls": [], "frames": [], "pos": -1}

T, H, W, N = 6, 50, 70, 8
SEED = 4321
THICKNESS, RADIUS, CROSS = 4, 8, 8
MARGIN = 1e-3


def install_stand_ins():
    cv2 = types.ModuleType("cv2")

    def line(img, pt1, pt2, color=None, thickness=None):
        LOG["calls"].append([LOG["pos"], 0, int(pt1[0]), int(pt1[1]), int(pt2[0]), int(pt2[1]), 0, int(thickness),
                             int(color[0]), int(color[1]), int(color[2]), LOG["frames"][-1]])
        return img

    def circle(img, center=None, radius=None, color=None, thickness=None):
        LOG["calls"].append([LOG["pos"], 1, int(center[0]), int(center[1]), int(center[0]), int(center[1]), int(radius),
                             int(thickness), int(color[0]), int(color[1]), int(color[2]), LOG["frames"][-1]])
        return img

    cv2.line, cv2.circle = line, circle

    tq = types.ModuleType("tqdm")

    def tqdm(items, *a, **k):
        for item in items:
            LOG["pos"] += 1
            LOG["frames"].append(int(item))
            yield item

    tq.tqdm = tqdm
    data_utils = types.ModuleType("data.data_utils")
    data_utils.load_video = data_utils.save_video = None
    utils = types.ModuleType("utils")
    utils.add_config_paths = None
    for m in (cv2, tq, data_utils, utils):
        sys.modules[m.__name__] = m
    sys.path.insert(0, ref_harness.REFERENCE_ROOT)


def scene():
    """(video, pred float32, gt float64, pred_occ, gt_occ): frame 0 by hand, the others seeded."""
    rng = np.random.default_rng(21)
    video = rng.integers(0, 256, size=(T, H, W, 3)).astype(np.uint8)
    gt = rng.uniform([4.0, 4.0], [W - 4.0, H - 4.0], size=(N, T, 2))
    pred = gt + rng.normal(0.0, 5.0, size=gt.shape)
    pocc = (rng.random((N, T)) < 0.3).astype(np.int32)
    gocc = (rng.random((N, T)) < 0.3).astype(bool)
    # frame 0: the four cases, an outside point, negative coordinates, pred = gt
    pred[:, 0] = [[10.7, 12.2], [30.2, 9.9], [48.6, 14.4], [20.0, 30.0], [90.5, 60.2], [-3.7, 5.9], [40.3, 35.8], [57.1, 40.6]]
    gt[:, 0] = [[20.3, 18.9], [33.0, 12.0], [55.4, 20.1], [22.0, 33.0], [85.0, 55.0], [2.5, -0.5], [40.9, 35.1], [63.9, 30.2]]
    pocc[:, 0] = [0, 0, 1, 1, 0, 0, 0, 1]
    gocc[:, 0] = [0, 1, 0, 1, 0, 0, 0, 0]
    # frame 1: a negative prediction under a cross and under a ring, a prediction far outside
    pred[1, 1], pocc[1, 1], gocc[1, 1] = [-0.9, -6.4], 0, 1
    pred[2, 1], pocc[2, 1], gocc[2, 1] = [-12.5, 20.5], 1, 0
    pred[4, 1], pocc[4, 1], gocc[4, 1] = [300.0, -200.0], 0, 0
    # frame 3: 6 of 8 ground-truth points below (1, 1) -- BADJA's `not annotated` -- the filter drops it; frame 4: 4 of 8, kept
    gt[:6, 3] = [[0, 0], [-1, -1], [0.5, 0.5], [0, 0.9], [0, 0], [-2, 0]]
    gt[:4, 4] = [[0, 0], [0, 0], [0.2, 0.3], [-1, 0]]
    gt[4, 4] = [0.5, 7.0]                 # only x below 1: not `below`
    return video, pred.astype(np.float32), gt, pocc, gocc


def badja_case():
    """A benchmark entry of one video (data/tapvid.py's format) and its predictions in the benchmark raster."""
    rng = np.random.default_rng(33)
    h, w, t_all, t_seg = 48, 64, 6, 5
    seg = np.zeros((t_seg, h, w), dtype=np.uint8)
    for t, side in enumerate((7, 10, 15, 20, 12)):          # areas 49 (unused frame 0), 100, 225, 400, 144
        seg[t, 3:3 + side, 5:5 + side] = (255, 1, 200, 7, 255)[t]
    thr = np.float32(0.2) * np.sqrt((seg > 0).reshape(t_seg, -1).sum(1).astype(np.float32))     # 1.4, 2, 3, 4, 2.4
    frames = [2, 0]                                          # the dict's order, not sorted
    sizes = {2: 5, 0: 7}
    target, occluded, pred = {}, {}, {}
    for f in frames:
        n = sizes[f]
        gt = rng.uniform([8.0, 8.0], [w - 8.0, h - 8.0], size=(n, t_all, 2))
        ang = rng.uniform(0, 2 * np.pi, size=(n, t_all))
        dist = rng.uniform(0.2, 6.0, size=(n, t_all))
        occ = rng.random((n, t_all)) < 0.25
        target[f], occluded[f] = gt, occ
        pred[f] = (gt, ang, dist)
    # distances just inside and just outside every threshold and 3.0, on visible entries
    edge = [(2, 0, 1, thr[1] - 0.01), (2, 1, 1, thr[1] + 0.01), (2, 2, 2, 3.0 - 0.02), (2, 3, 2, 3.0 + 0.02),
            (0, 0, 3, thr[3] - 0.01), (0, 1, 3, thr[3] + 0.01), (0, 2, 4, thr[4] - 0.01), (0, 3, 4, thr[4] + 0.01),
            (0, 4, 1, 3.0 - 0.01), (0, 5, 1, 3.0 + 0.01)]
    for f, i, t, d in edge:
        pred[f][2][i, t] = d
        occluded[f][i, t] = False
    out = {}
    for f in frames:
        gt, ang, dist = pred[f]
        out[f] = (gt + dist[..., None] * np.stack([np.cos(ang), np.sin(ang)], axis=-1)).astype(np.float32)
    config = {"video_idx": 0, "h": h, "w": w, "target_points": target, "occluded": occluded, "segmentations": seg,
              "query_points": {f: target[f][:, f] for f in frames}}
    return config, out, thr


def badja_margins(config, preds, thr, scale):
    """the float64 distances of the visible, scored entries against 3.0 and their frame's threshold."""
    sx, sy = np.float32(scale[0]), np.float32(scale[1])
    seen = {k: [False, False] for k in [("3px", None)] + [("thr", t) for t in range(1, len(thr))]}
    for f, gt in config["target_points"].items():
        p = preds[f].copy()
        p[..., 0] *= sx
        p[..., 1] *= sy
        d = np.sqrt(((p.astype(np.float64) - gt) ** 2).sum(-1))
        for t in range(1, len(thr)):
            dv = d[:, t][~config["occluded"][f][:, t]]
            for key, edge in ((("3px", None), 3.0), (("thr", t), float(thr[t]))):
                gap = dv - edge
                assert (np.abs(gap) >= MARGIN).all(), (f, t, key, float(np.abs(gap).min()))
                seen[key][0] |= bool(((gap < 0) & (gap > -0.05)).any())
                seen[key][1] |= bool(((gap > 0) & (gap < 0.05)).any())
    return seen


def main():
    install_stand_ins()
    P = importlib.import_module("visualization.visualize_pred_vs_gt")
    U = importlib.import_module("visualization.viz_utils")
    M = importlib.import_module("eval.metrics")
    assert ref_harness.REFERENCE_ROOT in P.__file__ and ref_harness.REFERENCE_ROOT in M.__file__
    out = {}

    # ---- (b) the picture --------------------------------------------------------------------------------------------------------
    video, pred, gt, pocc, gocc = scene()
    out.update(scene_video=video, scene_pred=pred, scene_gt=gt, scene_pred_occ=pocc, scene_gt_occ=gocc.astype(np.uint8),
               scene_seed=np.array(SEED), thickness=np.array(THICKNESS), radius=np.array(RADIUS), cross_size=np.array(CROSS))
    for name, badja in (("plain", False), ("badja", True)):
        LOG.update(calls=[], frames=[], pos=-1)
        np.random.seed(SEED)
        res = P.visualize_trajectories_with_gt(video, pred, gt, pocc, gocc, thickness=THICKNESS, radius=RADIUS, cross_size=CROSS,
                                               badja_vis_type=badja)
        assert res.shape == (len(LOG["frames"]), H, W, 3)
        np.testing.assert_array_equal(res, video[LOG["frames"]])                     # the stand-in draws nothing
        out[f"calls_{name}"] = np.array(LOG["calls"], dtype=np.int64).reshape(-1, 12)
        out[f"kept_{name}"] = np.array(LOG["frames"], dtype=np.int64)
    assert list(out["kept_plain"]) == list(range(T)) and list(out["kept_badja"]) == [0, 1, 2, 4, 5]
    np.random.seed(SEED)
    out["colors_plain"] = np.array(U.get_colors(N, seed=0, without_red=False), dtype=np.int64)
    np.random.seed(SEED)
    out["colors_without_red"] = np.array(U.get_colors(N, seed=0, without_red=True), dtype=np.int64)
    assert (out["colors_plain"] != out["colors_without_red"]).any(), "no colour is red enough for without_red to matter"
    # the scene has what its docstring says
    f0 = list(zip(pocc[:, 0] != 0, gocc[:, 0] != 0))
    assert {(False, False), (False, True), (True, False), (True, True)} <= set(f0)
    assert (pred[:, 0].astype(int) != np.floor(pred[:, 0]).astype(int)).any() and (gt[:, 0].astype(int) != np.floor(gt[:, 0]).astype(int)).any()
    c0 = out["calls_plain"][out["calls_plain"][:, 0] == 0]
    assert ((c0[:, 1] == 0) & (c0[:, 2] == c0[:, 4]) & (c0[:, 3] == c0[:, 5]) & (c0[:, 8] == 255)).any(), "no zero-length line"
    assert (c0[:, 2] >= W).any() and (c0[:, 2] < 0).any()
    kinds = {(int(r[1]), int(r[7])) for r in out["calls_plain"]}
    assert kinds == {(0, THICKNESS), (0, THICKNESS // 2), (1, -1), (1, 2)}, kinds

    # ---- (a) BADJA ----------------------------------------------------------------------------------------------------------------
    config, preds, thr = badja_case()
    h, w = config["h"], config["w"]
    bench = {"videos": [config]}
    big = {f: (p / np.array([np.float32(w / 854), np.float32(h / 476)], dtype=np.float32)).astype(np.float32) for f, p in preds.items()}
    for name, arrays, sizes, scale in (("none", preds, None, (1.0, 1.0)), ("854", big, [854, 476], (w / 854, h / 476))):
        seen = badja_margins(config, arrays, thr, scale)
        assert all(a and b for a, b in seen.values()), (name, seen)
        with tempfile.TemporaryDirectory() as d:
            for f, p in arrays.items():
                np.save(os.path.join(d, f"trajectories_{f}.npy"), p)
            m = M.compute_badja_metrics_for_video(d, bench, 0, pred_video_sizes=sizes)
        out[f"badja_acc_{name}"] = np.array([m["acc_seg"], m["acc_3px"]], dtype=np.float64)
        for f, p in arrays.items():
            out[f"badja_pred_{name}_{f}"] = p
        print(f"BADJA pred_video_sizes={sizes}: acc_seg {m['acc_seg']:.6f}  acc_3px {m['acc_3px']:.6f}")
    out["badja_frames"] = np.array(list(config["target_points"]), dtype=np.int64)
    for f in config["target_points"]:
        out[f"badja_gt_{f}"] = config["target_points"][f]
        out[f"badja_occ_{f}"] = config["occluded"][f].astype(np.uint8)
    out.update(badja_seg=config["segmentations"], badja_h=np.array(h), badja_w=np.array(w))
    assert all(v.dtype != object for v in out.values())
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT} ({size / 1024:.0f} KiB); calls: plain {len(out['calls_plain'])}, badja {len(out['calls_badja'])}")
    assert size < 1 << 20


if __name__ == "__main__":
    main()
