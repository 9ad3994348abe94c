"""GPU: the track-video rasteriser (csrc/render.hip, dino_tracker_amd/visualize.py) against the float64 restatement of the picture
in tests/viz_ref.py, stage by stage and end to end on the golden scene of tests/golden/viz.npz.

Bounds (docs/PARITY.md, "Track videos"): FOUR times the float32-against-float64 difference of viz_ref itself on the same inputs
(a different operation order and fused multiply-adds on the device), rounded up to two digits.  The differences are computed on the
CPU by tests/test_viz_reference.py::test_float32_against_float64, which also checks the numbers below against them."""
import os

import numpy as np
import pytest
import torch

import viz_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viz.npz")

# docs/PARITY.md "Track videos": 4 x the measured float32-against-float64 differences of viz_ref
COORD_BOUND = 4.5e-5         # pixels, record coordinates and sizes of the golden scene
ALPHA_BOUND = 3.1e-7         # record alphas of the golden scene
GOLDEN_BLEND_BOUND = 1.5e-5  # blended values in [0, 1], golden scene (trail and dotted videos)
NUMERIC_BLEND_BOUND = 9.6e-7 # blended values in [0, 1], the 300 random primitives


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def scene(gold):
    """The golden scene on the device plus its float64 reference records per frame (computed once, never modified)."""
    T, H, W = gold["video"].shape[:3]
    maps = R.frame_maps(gold["homogs"])
    ps, lw = int(gold["point_size"]), float(gold["linewidth"])
    tails = [R.tail_prims(gold["fg_pts"], gold["fg_occ"], maps, H, W, i, ps, lw, marker="D") for i in range(T)]
    dotted = [R.dotted_prims(gold["fg_pts"], gold["fg_occ"], H, W, i, ps, marker="o") for i in range(T)]
    for r in tails + dotted:
        r.setflags(write=False)
    return dict(T=T, H=H, W=W, ps=ps, lw=lw, tails=tails, dotted=dotted, maps32=maps.reshape(T, T, 9).astype(np.float32))


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host_records(t):
    """device records -> float64 [P, 12] with kind and frame as numbers."""
    raw = t.cpu().numpy()
    out = raw.astype(np.float64)
    bits = raw.view(np.int32)
    out[:, 0], out[:, 11] = bits[:, 0], bits[:, 11]
    return out


def check_blend(u8, f32, ref64, bound, what):
    """The rules of the numeric blend: float32 within `bound` of float64; uint8 at most one level off, and equal wherever 255 c of
    the float64 result lies further than 255 bound from a rounding boundary.  No share of pixels is exempted."""
    err = float(np.abs(f32.astype(np.float64) - ref64).max())
    want = R.to_u8(ref64)
    level = np.abs(u8.astype(np.int32) - want.astype(np.int32))
    scaled = 255.0 * ref64
    safe = np.abs(scaled - (np.floor(scaled) + 0.5)) > 255.0 * bound
    print(f"{what}: max |f32 - f64| {err:.3e} (bound {bound:.3e}); uint8 levels off: max {int(level.max())}, "
          f"{int((level > 0).sum())} of {level.size} values differ, {int((~safe).sum())} values within the bound of a rounding boundary")
    assert err <= bound
    assert level.max() <= 1
    assert (level[safe] == 0).all()


# ---- 1. primitives ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["tails", "dotted"])
def test_primitives_against_the_restatement(gold, scene, mode):
    """dtk_render_prims, every frame i of the golden scene, one frame per call and all frames in one call."""
    from dino_tracker_amd import ops, visualize as V
    T, H, W = scene["T"], scene["H"], scene["W"]
    pts, occ = dev(gold["fg_pts"]), dev(gold["fg_occ"] != 0, torch.uint8)
    colors = dev(R.rainbow(pts.shape[0]), torch.float32)
    tails = mode == "tails"
    args = dict(mode=ops.RENDER_TAILS if tails else ops.RENDER_DOTTED, marker_kind=ops.RENDER_DIAMOND if tails else ops.RENDER_DISC,
                marker_size=V.marker_size("D" if tails else "o", scene["ps"]), half_width=scene["lw"] * V.PX_PER_POINT / 2)
    maps = dev(scene["maps32"]) if tails else None
    whole = host_records(ops.render_prims(pts, occ, colors, maps, 0, T, H, W, **args))
    at, worst_xy, worst_a = 0, 0.0, 0.0
    for i in range(T):
        want = scene[mode][i]
        got = host_records(ops.render_prims(pts, occ, colors, maps, i, 1, H, W, **args))
        assert got.shape == want.shape
        np.testing.assert_array_equal(got[:, 0], want[:, 0])
        assert (got[:, 11] == 0).all()
        np.testing.assert_array_equal(got[:, 9] == 0, want[:, 9] == 0)          # the same primitives draw nothing
        worst_xy = max(worst_xy, float(np.abs(got[:, 1:6] - want[:, 1:6]).max()))
        worst_a = max(worst_a, float(np.abs(got[:, 9] - want[:, 9]).max()))
        assert np.abs(got[:, 6:9] - want[:, 6:9]).max() < 1e-7                  # colours: float32(float64 colour)
        rel = np.abs(got[:, 10] - want[:, 10]) / np.maximum(want[:, 10], 1e-30)
        longer = (want[:, 10] > 0) & (want[:, 10] < 100)                        # segments longer than 0.1 px
        assert (rel[longer] < 1e-3).all() and (got[:, 10][want[:, 10] == 0] == 0).all()
        part = whole[at:at + len(want)]
        assert (part[:, 11] == i).all()
        np.testing.assert_array_equal(part[:, :11], got[:, :11])                # grouping changes the frame index only
        at += len(want)
    assert at == len(whole)
    print(f"{mode}: max |coordinate diff| {worst_xy:.3e} px (bound {COORD_BOUND:.3e}), max |alpha diff| {worst_a:.3e} "
          f"(bound {ALPHA_BOUND:.3e})")
    assert worst_xy <= COORD_BOUND and worst_a <= ALPHA_BOUND


# ---- 2. exact ordering -----------------------------------------------------------------------------------------------------------
def test_tile_counts_and_keys():
    """The binning stages on their own: counts equal the tiles of the grown, clipped bounding box; the keys are unique, name
    exactly those tiles, and ascending order inside a tile is record order."""
    from dino_tracker_amd import ops
    frames, rec = R.exact_scene()
    F, H, W = frames.shape[:3]
    d = dev(R.device_records(rec))
    counts = ops.render_tile_counts(d, F, H, W).cpu().numpy()
    grow = rec[:, 5].astype(np.float64) + np.where(rec[:, 0] == R.DIAMOND, np.float64(np.float32(0.70711)), 0.5)
    lo = np.minimum(rec[:, 1:3], rec[:, 3:5]) - grow[:, None]
    hi = np.maximum(rec[:, 1:3], rec[:, 3:5]) + grow[:, None]
    lim = np.array([W - 1, H - 1], dtype=np.float64)
    visible = (hi >= 0).all(axis=1) & (lo <= lim).all(axis=1)
    t0 = np.floor(np.maximum(lo, 0)).astype(np.int64) // 16
    t1 = np.ceil(np.minimum(hi, lim)).astype(np.int64) // 16
    want = np.where(visible, (t1 - t0 + 1).prod(axis=1), 0)
    np.testing.assert_array_equal(counts, want)
    assert counts[0] == 5 * 4 and (counts[601:604] == 0).all()                  # the diagonal meets every tile; outside: none
    ends = torch.cumsum(dev(counts), 0, dtype=torch.int64)
    K = int(ends[-1])
    keys = ops.render_tile_keys(d, (ends - dev(counts)).contiguous(), K, F, H, W).cpu().numpy()
    assert len(np.unique(keys)) == K
    tile, p = keys >> 32, keys & 0xFFFFFFFF
    assert (tile < 20).all() and (np.bincount(p, minlength=len(rec)) == counts).all()      # frame 0 only; one key per met tile
    srt = np.sort(keys)
    assert (np.diff(srt) > 0).all()
    starts = ops.render_tile_starts(dev(srt), F, H, W).cpu().numpy()
    assert starts[0] == 0 and starts[20] == K and (starts[20:] == K).all() and len(starts) == 2 * 20 + 1
    inside = (srt >> 32) == 1 * 5 + 1                                           # tile (ty 1, tx 1) holds the 600 (+ the diagonal)
    assert inside.sum() >= 600 > 2 * ops.RENDER_CHUNK


def test_exact_ordering():
    """Opaque primitives on integer coordinates, 70 x 50: wherever the float64 picture is a pure selection (viz_ref.exact_mask)
    the uint8 output is BIT-EQUAL to viz_ref; frame 1 has no primitive and equals its input."""
    from dino_tracker_amd import ops
    frames, rec = R.exact_scene()
    u8, f32 = ops.render_records(dev(frames), dev(R.device_records(rec)), want_float=True)
    u8, f32 = u8.cpu().numpy(), f32.cpu().numpy()
    ref = R.blend(frames[0], rec)
    mask = R.exact_mask(frames.shape[1:3], rec)
    print(f"exact ordering: {int(mask.sum())} of {mask.size} pixels compared bit for bit; max |f32 - f64| anywhere "
          f"{np.abs(f32[0] - ref).max():.3e}")
    assert mask.mean() > 0.8 and mask[16:32, 16:32].mean() > 0.4               # the crowded tile is compared too
    np.testing.assert_array_equal(u8[0][mask], R.to_u8(ref)[mask])
    np.testing.assert_array_equal(f32[0][mask], ref.astype(np.float32)[mask])
    np.testing.assert_array_equal(u8[1], frames[1])
    assert (u8[0] != frames[0]).any(axis=-1)[16:32, 16:32].mean() > 0.5


def test_exact_single_point():
    """N = 1 through dtk_render_prims: integer track, identity maps, no fade -- axis-aligned opaque segments."""
    from dino_tracker_amd import ops, visualize as V
    H, W, T = 50, 70, 4
    pts = np.array([[[10, 10], [30, 10], [30, 40], [65, 40]]], dtype=np.float32)
    occ = np.zeros((1, T), dtype=np.uint8)
    frames = np.random.default_rng(2).integers(0, 256, size=(T, H, W, 3)).astype(np.uint8)
    homogs = np.stack([np.eye(3)] * T)
    col = np.array([[1.0, 0.25, 0.0]])
    out = V.plot_tracks_tails(dev(frames), dev(pts), dev(occ), homogs, point_size=81, linewidth=72 / 64 * 3, marker="o",
                              colors_arr=col, trail_fade=False).cpu().numpy()
    maps = R.frame_maps(homogs)
    for i in range(T):
        rec = R.tail_prims(pts, occ, maps, H, W, i, 81, 72 / 64 * 3, marker="o", colors=col, trail_fade=False)
        assert rec[0, 5] == 4.0 and (i == 0 or rec[1, 5] == 1.5) and (rec[:, 9] == 1).all()
        mask = R.exact_mask((H, W), rec)
        np.testing.assert_array_equal(out[i][mask], R.to_u8(R.blend(frames[i], rec))[mask])
        assert mask.mean() > 0.9


# ---- 3. numeric blend ------------------------------------------------------------------------------------------------------------
def test_numeric_blend():
    """300 random primitives of the three kinds with a in (0, 1) on 80 x 50."""
    from dino_tracker_amd import ops
    frame, rec = R.numeric_scene()
    u8, f32 = ops.render_records(dev(frame[None]), dev(R.device_records(rec)), want_float=True)
    check_blend(u8[0].cpu().numpy(), f32[0].cpu().numpy(), R.blend(frame, rec), NUMERIC_BLEND_BOUND, "numeric blend")


# ---- 4. reproducibility ----------------------------------------------------------------------------------------------------------
def test_reproducible_and_independent_of_the_frame_groups(gold):
    from dino_tracker_amd import visualize as V
    v, p, o = dev(gold["video"]), dev(gold["fg_pts"]), dev(gold["fg_occ"])
    kw = dict(point_size=int(gold["point_size"]), linewidth=float(gold["linewidth"]), marker="D")
    stats = {}
    a = V.plot_tracks_tails(v, p, o, gold["homogs"], stats=stats, **kw)
    b = V.plot_tracks_tails(v, p, o, gold["homogs"], **kw)
    c = V.plot_tracks_tails(v, p, o, gold["homogs"], group_frames=1, **kw)
    d = V.plot_tracks_tails(v, p, o, gold["homogs"], group_frames=4, **kw)
    assert stats["groups"] == 1 and stats["prims"] == 9 * 21
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    # a tiny budget still renders (one frame per group) and changes nothing
    stats = {}
    e = V.plot_tracks_tails(v, p, o, gold["homogs"], memory_budget=1, stats=stats, **kw)
    assert stats["groups"] == 6 and torch.equal(a, e)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
def test_end_to_end_trails(gold, scene):
    from dino_tracker_amd import visualize as V
    u8, f32 = V.plot_tracks_tails(gold["video"], gold["fg_pts"], gold["fg_occ"], gold["homogs"], point_size=scene["ps"],
                                  linewidth=scene["lw"], marker="D", return_float=True)
    assert isinstance(u8, np.ndarray) and u8.dtype == np.uint8 and u8.shape == gold["video"].shape
    ref = np.stack([R.blend(gold["video"][i], scene["tails"][i]) for i in range(scene["T"])])
    check_blend(u8, f32, ref, GOLDEN_BLEND_BOUND, "trail video")
    assert (u8 != gold["video"]).any()


def test_end_to_end_dotted(gold, scene):
    from dino_tracker_amd import visualize as V
    u8, f32 = V.plot_tracks_v2(dev(gold["video"]), dev(gold["fg_pts"]), dev(gold["fg_occ"]), rainbow_colors=True,
                               point_size=scene["ps"], return_float=True)
    assert isinstance(u8, torch.Tensor) and u8.is_cuda and u8.dtype == torch.uint8
    ref = np.stack([R.blend(gold["video"][i], scene["dotted"][i]) for i in range(scene["T"])])
    check_blend(u8.cpu().numpy(), f32.cpu().numpy(), ref, GOLDEN_BLEND_BOUND, "dotted video")


def test_refusals(gold):
    from dino_tracker_amd import ops, visualize as V
    v, p, o = gold["video"], gold["fg_pts"], gold["fg_occ"]
    for kw in (dict(rainbow_colors=False), dict(rainbow_colors=True, gt_points=p), dict(rainbow_colors=True, trackgroup=np.arange(9)),
               dict(rainbow_colors=True, show_pred_occluded=True)):
        with pytest.raises(NotImplementedError):
            V.plot_tracks_v2(v, p, o, **kw)
    with pytest.raises(NotImplementedError):
        V.plot_tracks_tails(v, p, o, gold["homogs"], marker="x")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.plot_tracks_tails(torch.from_numpy(v), p, o, gold["homogs"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_tile_counts(torch.zeros(4, 12), 1, 50, 80)
    with pytest.raises(RuntimeError, match="marker_kind"):
        ops.render_prims(dev(p), dev(o != 0, torch.uint8), dev(R.rainbow(9), torch.float32), None, 0, 1, 50, 80, ops.RENDER_DOTTED,
                         ops.RENDER_SEGMENT, 3.0)
    with pytest.raises(RuntimeError, match="frame-to-frame maps"):
        ops.render_prims(dev(p), dev(o != 0, torch.uint8), dev(R.rainbow(9), torch.float32), None, 0, 1, 50, 80, ops.RENDER_TAILS,
                         ops.RENDER_DISC, 3.0)
    with pytest.raises(RuntimeError, match="bad sizes"):
        ops.render_prims(dev(p), dev(o != 0, torch.uint8), dev(R.rainbow(9), torch.float32), None, 4, 3, 50, 80, ops.RENDER_DOTTED,
                         ops.RENDER_DISC, 3.0)


def test_cli_writes_both_videos(tmp_path, capsys):
    """python -m dino_tracker_amd.visualize on a synthetic data folder (viz_data.write_data_folder), run in this process through
    its argument parser: the dotted and the rainbow video are written (mp4 with imageio, PNG frames without) and say so."""
    import viz_data as D
    from dino_tracker_amd import visualize as V
    root = D.write_data_folder(str(tmp_path / "scene"))
    args = V.make_parser().parse_args(["--data-path", root, "--infer-res-size", "50", "80", "--of-res-size", "50", "80",
                                       "--plot-trails", "--erosion-kernel-size", "3", "--fps", "5"])
    np.random.seed(0)
    torch.manual_seed(0)
    written = V.run(args)
    said = capsys.readouterr().out
    assert len(written) == 2 and all(os.path.exists(w) for w in written) and said.count("save_video:") == 2
    assert "dotted_tracks_erosion_kernel_3_fps_5" in written[0] and "rainbow_erosion_kernel_3_fps_5" in written[1]
    for w in written:
        if os.path.isdir(w):
            from PIL import Image
            files = sorted(os.listdir(w))
            assert len(files) == D.T
            frame = np.asarray(Image.open(os.path.join(w, files[-1])))
            assert frame.shape == (D.H, D.W, 3) and (frame != D.video()[-1]).any()
