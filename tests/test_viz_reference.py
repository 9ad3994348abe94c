"""CPU: the host half of dino_tracker_amd/visualize.py and the picture definition of tests/viz_ref.py against the reference calls
recorded in tests/golden/viz.npz (make_golden_viz.py: the unmodified viz_utils_tapir.py with drawing stand-ins).

test_float32_against_float64 computes the float32-against-float64 differences of viz_ref on the inputs of tests/test_gpu_render.py;
four times those are the device bounds hard-coded there (docs/PARITY.md)."""
import os

import numpy as np
import pytest
import torch

import viz_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viz.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def normalised(h):
    """each 3 x 3 divided by its Frobenius norm, sign fixed by its largest entry."""
    h = np.asarray(h, dtype=np.float64)
    h = h / np.linalg.norm(h, axis=(-2, -1), keepdims=True)
    flat = h.reshape(len(h), 9)
    big = flat[np.arange(len(h)), np.abs(flat).argmax(axis=1)]
    return h * np.sign(big)[:, None, None]


def test_homographies_reproduce_the_reference(gold):
    """Same draws from np.random in the same order, same arithmetic, same LAPACK: only operation order may differ."""
    from dino_tracker_amd import visualize as V
    np.random.seed(int(gold["seed"]))
    homogs, err, canonical = V.get_homographies_wrt_frame(gold["bg_pts"], gold["bg_occ"], [80, 50], thresh=0.07,
                                                          outlier_point_threshold=0.95, num_refinement_passes=2)
    d = np.abs(normalised(homogs) - normalised(gold["homogs"])).max()
    print(f"homographies: max |diff| of the normalised matrices {d:.3e}; err {np.abs(err - gold['err']).max():.3e}; "
          f"canonical {np.abs(canonical - gold['canonical']).max():.3e}")
    assert d < 1e-9
    np.testing.assert_allclose(err, gold["err"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(canonical, gold["canonical"], rtol=0, atol=1e-9)
    # an explicit generator with the same stream gives the same result
    h2, _, _ = V.get_homographies_wrt_frame(gold["bg_pts"], gold["bg_occ"], [80, 50], rng=np.random.RandomState(int(gold["seed"])))
    assert np.abs(normalised(h2) - normalised(gold["homogs"])).max() < 1e-9


def test_trail_primitives_equal_the_recorded_calls(gold):
    """viz_ref's markers, segments and alphas (float64) are the reference's scatter / LineCollection arguments, in its order."""
    T, H, W = gold["video"].shape[:3]
    pts, occ = gold["fg_pts"], gold["fg_occ"]
    N = pts.shape[0]
    maps = R.frame_maps(gold["homogs"])
    worst = 0.0
    for i in range(T):
        rec = R.tail_prims(pts, occ, maps, H, W, i, int(gold["point_size"]), float(gold["linewidth"]), marker="D")
        assert rec.shape == (N * (i + 1), 12)
        mk, seg = rec[:N], rec[N:].reshape(i, N, 12)
        assert (mk[:, 0] == R.DIAMOND).all() and (seg[..., 0] == R.SEGMENT).all()
        got_seg = np.stack([seg[..., 1:3], seg[..., 3:5]], axis=2)              # [i, N, 2 ends, 2]
        for a, b in ((mk[:, 1:3], gold["tails_scatter_xy"][i]), (mk[:, 6:10], gold["tails_scatter_c"][i]),
                     (got_seg, gold[f"tails_seg_{i}"]), (seg[..., 6:10], gold[f"tails_col_{i}"])):
            if a.size:
                worst = max(worst, float(np.abs(a - b).max()))
    print(f"trail primitives: max |diff| to the recorded reference arguments {worst:.3e}")
    assert worst < 1e-9
    # sizes: matplotlib's conventions at 64 dpi
    assert rec[0, 5] == pytest.approx(np.sqrt(40.0) * (64 / 72) * np.sqrt(2) / 2) and rec[-1, 5] == pytest.approx(1.5 * (64 / 72) / 2)


def test_dotted_primitives_equal_the_recorded_calls(gold):
    T, H, W = gold["video"].shape[:3]
    worst = 0.0
    for i in range(T):
        rec = R.dotted_prims(gold["fg_pts"], gold["fg_occ"], H, W, i, int(gold["point_size"]), marker="o")
        assert (rec[:, 0] == R.DISC).all()
        worst = max(worst, float(np.abs(rec[:, 1:3] - gold["v2_scatter_xy"][i]).max()),
                    float(np.abs(rec[:, 6:10] - gold["v2_scatter_c"][i]).max()))
    assert worst < 1e-9


def test_package_colours_sizes_and_maps_are_the_restatement(gold):
    from dino_tracker_amd import visualize as V
    np.testing.assert_array_equal(V.rainbow_colors(9), R.rainbow(9))
    for marker in "oD":
        assert V.marker_size(marker, 40) == float(R.marker_size(marker, 40))
    np.testing.assert_array_equal(V.frame_maps(gold["homogs"]).reshape(6, 6, 3, 3), R.frame_maps(gold["homogs"]).astype(np.float32))
    with pytest.raises(NotImplementedError):
        V.marker_size("x", 40)


@pytest.mark.parametrize("k", [1, 3, 5])
def test_erosion_is_a_min_filter_with_a_geodesic_border(k):
    """-max_pool2d(-m, k, 1, k // 2) against a direct minimum over the k x k window clipped to the image (pixels beyond the edge
    do not take part), on a mask that touches the border."""
    from dino_tracker_amd import visualize as V
    rng = np.random.default_rng(k)
    m = (rng.random((13, 17)) < 0.8).astype(np.float32)
    m[0:3, :9] = 1
    m[:, -1] = 1
    m[5:9, 0:3] = 1
    want = np.empty_like(m)
    r = k // 2
    for y in range(m.shape[0]):
        for x in range(m.shape[1]):
            want[y, x] = m[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1].min()
    got = V.erode_mask(torch.from_numpy(m), k).numpy()
    np.testing.assert_array_equal(got, want)
    assert k == 1 or (got[0, 2:7].sum() > 0 and got.sum() < m.sum())


def test_erosion_refuses_even_kernels():
    from dino_tracker_amd import visualize as V
    for k in (0, 2, 4):
        with pytest.raises(ValueError, match="odd"):
            V.erode_mask(torch.ones(4, 4), k)


def test_unimplemented_options_raise_without_a_device(gold):
    from dino_tracker_amd import visualize as V
    v, p, o = gold["video"], gold["fg_pts"], gold["fg_occ"]
    for kw in (dict(rainbow_colors=False), dict(rainbow_colors=True, gt_points=p), dict(rainbow_colors=True, trackgroup=np.arange(9)),
               dict(rainbow_colors=True, show_pred_occluded=True)):
        with pytest.raises(NotImplementedError):
            V.plot_tracks_v2(v, p, o, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.plot_tracks_v2(torch.from_numpy(v), p, o, rainbow_colors=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.plot_tracks_tails(torch.from_numpy(v), p, o, gold["homogs"])


def test_filter_bg_trajectories_follows_randperm():
    """The selection is the reference's: per frame, the first 500 // T entries of torch.randperm over the long valid tracks."""
    from dino_tracker_amd import visualize as V
    g = torch.Generator().manual_seed(3)
    bg = torch.rand(60, 12, 2, generator=g) * 50
    bg[torch.rand(60, 12, generator=g) < 0.1] = float("nan")
    torch.manual_seed(5)
    got = V.filter_bg_trajectories_for_homographies(bg, bg_trajectories_count=48, canonical_frame=None, min_len=8)
    torch.manual_seed(5)
    valid = ~bg.isnan().any(-1)
    picked = []
    for t in range(12):
        idx = torch.where((valid.sum(-1) * (valid[:, t] & valid[:, 6]).float()) > 8)[0]
        assert len(idx) >= 4
        picked.append(idx[torch.randperm(len(idx))[:4]])
    want = bg[torch.unique(torch.cat(picked))]
    assert got.shape == want.shape and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))


def float32_differences(gold):
    """{name: max |float32 run - float64 run| of viz_ref} on the inputs of the GPU tests."""
    T, H, W = gold["video"].shape[:3]
    pts, occ, video = gold["fg_pts"], gold["fg_occ"], gold["video"]
    maps = R.frame_maps(gold["homogs"])
    ps, lw = int(gold["point_size"]), float(gold["linewidth"])
    out = {"coord": 0.0, "alpha": 0.0, "golden_blend": 0.0}
    for i in range(T):
        r64 = R.tail_prims(pts, occ, maps, H, W, i, ps, lw, marker="D")
        r32 = R.tail_prims(pts, occ, maps, H, W, i, ps, lw, marker="D", dtype=np.float32)
        assert ((r64[:, 9] == 0) == (r32[:, 9] == 0)).all()                     # the discrete decisions agree
        out["coord"] = max(out["coord"], float(np.abs(r32[:, 1:6] - r64[:, 1:6]).max()))
        out["alpha"] = max(out["alpha"], float(np.abs(r32[:, 9] - r64[:, 9]).max()))
        out["golden_blend"] = max(out["golden_blend"], float(np.abs(R.blend(video[i], r32, np.float32) - R.blend(video[i], r64)).max()))
        d64 = R.dotted_prims(pts, occ, H, W, i, ps)
        d32 = R.dotted_prims(pts, occ, H, W, i, ps, dtype=np.float32)
        out["coord"] = max(out["coord"], float(np.abs(d32[:, 1:6] - d64[:, 1:6]).max()))
        out["golden_blend"] = max(out["golden_blend"], float(np.abs(R.blend(video[i], d32, np.float32) - R.blend(video[i], d64)).max()))
    frame, rec = R.numeric_scene()
    out["numeric_blend"] = float(np.abs(R.blend(frame, rec, np.float32) - R.blend(frame, rec)).max())
    return out


def test_float32_against_float64(gold):
    """The measured differences, printed; the device bounds of tests/test_gpu_render.py are FOUR times these (a different operation
    order and fused multiply-adds), rounded up to two digits -- checked here so that the hard-coded numbers cannot drift."""
    import test_gpu_render as G
    d = float32_differences(gold)
    print("float32 against float64 (viz_ref):", {k: f"{v:.3e}" for k, v in d.items()})
    for name, bound in (("coord", G.COORD_BOUND), ("alpha", G.ALPHA_BOUND), ("golden_blend", G.GOLDEN_BLEND_BOUND),
                        ("numeric_blend", G.NUMERIC_BLEND_BOUND)):
        assert 4 * d[name] <= bound <= 4 * d[name] * 1.05, (name, d[name], bound)
