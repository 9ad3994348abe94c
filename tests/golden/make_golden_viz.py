"""Writes tests/golden/viz.npz by running the UN-MODIFIED reference visualization/viz_utils_tapir.py on the inputs of viz_data.py
(needs a reference checkout, oracle/ref_harness.py REFERENCE_ROOT):
    python tests/golden/make_golden_viz.py

The module imports matplotlib, matplotlib.pyplot, matplotlib.collections and mediapy; this generator puts stand-ins for the four
into sys.modules first.  The stand-ins draw NOTHING: plt.cm.hsv returns the colorsys colours (docs/RENDER.md: matplotlib's map is a
256-entry table of the same ramp), plt.scatter and LineCollection record their arguments, the canvas returns a blank image.  What
is recorded is therefore the reference's GEOMETRY, DRAW ORDER and ALPHAS -- the part of the picture that is the reference's.

Stored: the inputs (video, bg_pts / bg_occ as get_homographies_wrt_frame receives them, fg_pts / fg_occ), the np.random seed, the
outputs of get_homographies_wrt_frame (homogs, err, canonical), and per frame i of plot_tracks_tails: tails_scatter_xy [T, N, 2],
tails_scatter_c [T, N, 4], tails_scatter_s, tails_seg_<i> [i, N, 2, 2] (LineCollection segments, newest pair first) and
tails_col_<i> [i, N, 4] (their rgba); of plot_tracks_v2: v2_scatter_xy, v2_scatter_c, v2_scatter_s.

Asserted here, so that tests can rely on the discrete decisions being the same in a float32 or reordered evaluation:
  * no squared error within 1e-6 (relative) of a threshold it is compared with (thresh^2 in compute_inliers and the refinement;
    thresh and 2 thresh in compute_canonical_points);
  * no inlier fraction within 1e-6 of required_inlier_frac;
  * no trail endpoint coordinate within 1e-3 px of 1, W or H -- except coordinates that ARE a clamp value (0, W or H exactly, from
    the clamp to [0, W] x [0, H]): those compare exactly in any precision.
"""
import colorsys
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import ref_harness  # noqa: E402
import viz_data as D  # noqa: E402

OUT = os.path.join(HERE, "viz.npz")
REL, PX = 1e-6, 1e-3
LOG = {"frames": []}


def install_stand_ins():
    mpl, plt, coll, media = (types.ModuleType(n) for n in ("matplotlib", "matplotlib.pyplot", "matplotlib.collections", "mediapy"))

    def hsv(z):
        return np.array([colorsys.hsv_to_rgb(float(v), 1.0, 1.0) + (1.0,) for v in np.asarray(z)], dtype=np.float64)

    class Axes:
        def axis(self, *a, **k): pass
        def imshow(self, img): LOG["frames"][-1]["image"] = np.asarray(img)
        def add_collection(self, c): LOG["frames"][-1]["lines"].append(c)

    class Canvas:
        def __init__(self, fig): self.fig = fig
        def draw(self): pass
        def tostring_rgb(self): return bytes(int(round(self.fig.size[0] * 64)) * int(round(self.fig.size[1] * 64)) * 3)

    class Figure:
        def __init__(self, figsize, dpi, **k):
            self.size, self.dpi, self.ax, self.canvas = np.array(figsize, dtype=np.float64), dpi, Axes(), Canvas(self)
        def add_subplot(self): return self.ax
        def get_size_inches(self): return self.size
        def get_dpi(self): return self.dpi

    class LineCollection:
        def __init__(self, segments, color=None, linewidth=None):
            self.segments, self.color, self.linewidth = np.array(segments), np.array(color), linewidth

    state = {}

    def figure(figsize=None, dpi=None, **k):
        LOG["frames"].append({"scatter": [], "lines": []})
        state["fig"] = Figure(figsize, dpi)
        return state["fig"]

    def scatter(x, y, s=None, c=None, marker=None, **k):
        LOG["frames"][-1]["scatter"].append({"x": np.array(x), "y": np.array(y), "s": s, "c": np.array(c), "marker": marker})

    plt.cm = types.SimpleNamespace(hsv=hsv)
    plt.figure, plt.scatter = figure, scatter
    plt.gca = lambda: state["fig"].ax
    plt.subplots_adjust = plt.margins = plt.close = lambda *a, **k: None
    coll.LineCollection = LineCollection
    mpl.pyplot, mpl.collections = plt, coll
    for m in (mpl, plt, coll, media):
        sys.modules[m.__name__] = m


def load_reference():
    path = os.path.join(ref_harness.REFERENCE_ROOT, "visualization", "viz_utils_tapir.py")
    spec = importlib.util.spec_from_file_location("viz_utils_tapir_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def away(values, threshold, what):
    gap = np.abs(np.asarray(values, dtype=np.float64) - threshold)
    assert (gap > REL * abs(threshold)).all(), (what, float(gap.min()), threshold)


def watch_margins(V):
    inliers, canonical = V.compute_inliers, V.compute_canonical_points

    def compute_inliers(homog, thresh, targ_pts=None, src_pts=None, src_pts_homog=None):
        res = inliers(homog, thresh, targ_pts=targ_pts, src_pts=src_pts, src_pts_homog=src_pts_homog)
        away(res[1], thresh * thresh, "squared error against thresh^2")
        return res

    def compute_canonical_points(all_tformed, occ, err, inner, outer, required):
        away(err, inner, "error against the inner threshold")
        away(err, outer, "error against the outer threshold")
        maybe = np.logical_and(np.logical_not(occ), err < inner)
        frac = np.sum(maybe, axis=0) / np.maximum(1.0, np.sum(np.logical_not(occ), axis=0))
        away(frac, required, "inlier fraction against required_inlier_frac")
        return canonical(all_tformed, occ, err, inner, outer, required)

    V.compute_inliers, V.compute_canonical_points = compute_inliers, compute_canonical_points


def main():
    install_stand_ins()
    V = load_reference()
    watch_margins(V)
    import contextlib
    import io

    bg, _ = D.background()
    bg_occ = np.isnan(bg).any(axis=-1).astype(np.int32)
    bg_pts = np.nan_to_num(bg, nan=0)
    fg_pts, fg_occ = D.foreground()
    video = D.video()
    out = {"video": video, "bg_pts": bg_pts, "bg_occ": bg_occ, "fg_pts": fg_pts, "fg_occ": fg_occ,
           "seed": np.array(D.NP_RANDOM_SEED), "point_size": np.array(D.POINT_SIZE), "linewidth": np.array(D.LINEWIDTH)}

    np.random.seed(D.NP_RANDOM_SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        homogs, err, canonical = V.get_homographies_wrt_frame(bg_pts, bg_occ, [D.W, D.H], thresh=0.07, outlier_point_threshold=0.95,
                                                              num_refinement_passes=2, reference_frame=None)
    out.update(homogs=homogs, err=err, canonical=canonical)
    # the estimate is a pan: frame-to-frame maps close to the cameras of viz_data (a sanity check of the scene, not a fixture)
    m = np.linalg.inv(homogs[5]) @ homogs[0]
    true = D.camera(5) @ np.linalg.inv(D.camera(0))
    print("map 0 -> 5, estimate / truth (normalised):\n", m / m[2, 2], "\n", true / true[2, 2])

    LOG["frames"] = []
    with contextlib.redirect_stdout(io.StringIO()):
        blank = V.plot_tracks_tails(video, fg_pts, fg_occ, homogs, point_size=D.POINT_SIZE, linewidth=D.LINEWIDTH, marker="D")
    assert blank.shape == video.shape and len(LOG["frames"]) == D.T
    lim = np.array([D.W, D.H], dtype=np.float64)
    for i, fr in enumerate(LOG["frames"]):
        (sc,) = fr["scatter"]
        assert sc["marker"] == "D" and sc["s"] == D.POINT_SIZE and len(fr["lines"]) == i
        np.testing.assert_array_equal(fr["image"], video[i] / 255.0)
        assert all(c.linewidth == D.LINEWIDTH for c in fr["lines"])
        seg = np.stack([c.segments for c in fr["lines"]]) if i else np.zeros((0, D.N_FG, 2, 2))
        col = np.stack([c.color for c in fr["lines"]]) if i else np.zeros((0, D.N_FG, 4))
        out[f"tails_seg_{i}"], out[f"tails_col_{i}"] = seg, col
    out["tails_scatter_xy"] = np.stack([np.stack([f["scatter"][0]["x"], f["scatter"][0]["y"]], axis=-1) for f in LOG["frames"]])
    out["tails_scatter_c"] = np.stack([f["scatter"][0]["c"] for f in LOG["frames"]])
    out["tails_scatter_s"] = np.array(D.POINT_SIZE)

    # the endpoint margin, on the UNCLAMPED endpoints (the recorded segments are clamped to [1, lim - 1])
    import viz_ref as R
    maps = R.frame_maps(homogs)
    pts = R.clamp_points(fg_pts, D.H, D.W, np.float64)
    worst = np.inf
    for i in range(D.T):
        for j in range(i + 1):
            if j == i:
                p = pts[:, i]
            else:
                q = np.concatenate([pts[:, j], np.ones((D.N_FG, 1))], axis=1) @ maps[i, j].T
                p = q[:, :2] / q[:, 2:]
            exact = (p == 0) | (p == lim)
            for edge in (1.0, lim):
                gap = np.where(exact, np.inf, np.abs(p - edge))
                worst = min(worst, float(gap.min()))
    assert worst > PX, worst
    print(f"closest endpoint coordinate to 1 / W / H: {worst:.4f} px")

    LOG["frames"] = []
    blank = V.plot_tracks_v2(video, fg_pts, fg_occ, rainbow_colors=True, point_size=D.POINT_SIZE)
    assert blank.shape == video.shape and len(LOG["frames"]) == D.T
    assert all(len(f["scatter"]) == 1 and f["scatter"][0]["marker"] == "o" and not f["lines"] for f in LOG["frames"])
    out["v2_scatter_xy"] = np.stack([np.stack([f["scatter"][0]["x"], f["scatter"][0]["y"]], axis=-1) for f in LOG["frames"]])
    out["v2_scatter_c"] = np.stack([f["scatter"][0]["c"] for f in LOG["frames"]])
    out["v2_scatter_s"] = np.array(D.POINT_SIZE)

    alphas = np.concatenate([out[f"tails_col_{i}"][..., 3].ravel() for i in range(D.T)])
    print(f"segments: {alphas.size}, of them a = 0: {(alphas == 0).sum()}; occluded fg entries {int(fg_occ.sum())}; "
          f"bg occluded {int(bg_occ.sum())} of {bg_occ.size}")
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT} ({size / 1024:.0f} KiB)")
    assert size < 1 << 20


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    main()
