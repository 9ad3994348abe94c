"""GPU: the four device steps between the tracker's first pass and its occlusion flags, each called through its ops wrapper on
operands the test owns and compared with the plain references of tests/anchor_stage_ref.py (pinned to the oracle by
tests/test_anchor_stage_reference.py): dtk_build_anchor_sources and dtk_occlusion (csrc/anchors.hip) exactly, at the chunk
boundaries of their scans and the lane strides of the median; dtk_traj_cos_sims, dtk_sample_points, dtk_sample_grid and the
layout / norm kernels (csrc/core.hip) against float64 at channel counts around the 256-float stride of a wave; the TAP-Vid counts
on the strict thresholds.  No Tracker is built and no decision is left out."""
import numpy as np
import pytest
import torch

import anchor_stage_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
SENTINEL = -7


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- dtk_build_anchor_sources --------------------------------------------------------------------------------------------------
SOURCE_SHAPES = [(1, 1), (1, 2), (5, 7), (255, 3), (256, 16), (257, 16), (513, 5), (3, 64), (3, 65), (2, 257), (3, 300)]
PATTERNS = ["uniform", "ones", "one_frame", "mixed"]
TH = R.ANCHOR_TH


def cs_pattern(pattern, N, T, seed):
    rng = np.random.default_rng(seed)
    if pattern == "uniform":
        return rng.random((N, T)).astype(np.float32)
    if pattern == "ones":
        return np.ones((N, T), dtype=np.float32)
    if pattern == "one_frame":
        cs = (rng.random((N, T)) * 0.69).astype(np.float32)
        cs[np.arange(N), rng.integers(0, T, N)] = 0.95
        return cs
    cs = rng.random((N, T)).astype(np.float32)
    cs[rng.random((N, T)) < 0.2] = np.float32(TH)  # exactly on the threshold: anchors
    cs[rng.random((N, T)) < 0.1] = np.nextafter(np.float32(TH), np.float32(0))  # one ulp below: not
    cs[rng.random((N, T)) < 0.15] = np.nan
    cs[::3] = np.minimum(np.nan_to_num(cs[::3], nan=0.0), 0.5)  # rows without any anchor (row 0 among them)
    return cs


def sentinel_buffers(N, T):
    from dino_tracker_amd import ops
    buf = ops.AnchorSources(N, T, DEV)
    for name in ("n_anchors", "pair_off", "pair_frame", "src_row", "tgt", "out_idx", "counts", "scratch"):
        getattr(buf, name).fill_(SENTINEL)
    return buf


def check_sources(buf, want, N, T, untouched_is_sentinel=True):
    P, M = int(want.counts[0]), int(want.counts[1])
    got_counts = buf.counts.cpu().numpy()
    assert got_counts[:3].tolist() == want.counts.tolist()
    assert np.array_equal(buf.n_anchors.cpu().numpy(), want.n_anchors)
    assert buf.pair_off.numel() == N + 1 and np.array_equal(buf.pair_off.cpu().numpy(), want.pair_off)
    assert np.array_equal(buf.pair_frame[:P].cpu().numpy(), want.pair_frame)
    for name in ("src_row", "tgt", "out_idx"):
        assert np.array_equal(getattr(buf, name)[:M].cpu().numpy(), getattr(want, name)), name
    if untouched_is_sentinel:
        assert got_counts[3] == SENTINEL
        assert (buf.pair_frame[P:] == SENTINEL).all()
        for name in ("src_row", "tgt", "out_idx"):
            assert getattr(buf, name).numel() == N * T * T and (getattr(buf, name)[M:] == SENTINEL).all(), name


@pytest.mark.parametrize("N,T", SOURCE_SHAPES)
def test_build_anchor_sources_exact(N, T):
    """every output equals the plain loops on its valid prefix -- pair_frame[:pairs], the three source lists [:pairs*T],
    pair_off[:N+1], counts[:3] -- and nothing behind the prefix is written; N crosses the 256-wide chunks of the query scan
    (255 / 256 / 257 / 513), T those of the frame scan (257, 300)"""
    from dino_tracker_amd import ops
    for i, pattern in enumerate(PATTERNS):
        cs = cs_pattern(pattern, N, T, 1000 * N + 10 * T + i)
        want = R.anchor_sources_ref(cs, TH)
        if pattern == "mixed":
            assert want.counts[2] > 0 and (N * T < 8 or ((cs == np.float32(TH)).any() and np.isnan(cs).any()))
        buf = sentinel_buffers(N, T)
        out = ops.build_anchor_sources(dev(cs), TH, buf)
        assert out is buf
        check_sources(buf, want, N, T)


def test_build_anchor_sources_reuses_its_buffers():
    """a dense call followed by a sparse one into the same buffers: the second result is right on its (shorter) prefix"""
    from dino_tracker_amd import ops
    N, T = 257, 16
    dense, sparse = cs_pattern("ones", N, T, 1), cs_pattern("mixed", N, T, 2)
    buf = sentinel_buffers(N, T)
    ops.build_anchor_sources(dev(dense), TH, buf)
    check_sources(buf, R.anchor_sources_ref(dense, TH), N, T)
    again = ops.build_anchor_sources(dev(sparse), TH, buf)
    assert again is buf
    want = R.anchor_sources_ref(sparse, TH)
    assert 0 < want.counts[0] < N * T and want.counts[2] > 0
    check_sources(buf, want, N, T, untouched_is_sentinel=False)


# ---- dtk_occlusion -------------------------------------------------------------------------------------------------------------
def device_occlusion(case):
    from dino_tracker_amd import ops
    return ops.occlusion(dev(case.green), dev(case.pair_off), dev(case.pair_frame), dev(case.traj), dev(case.cs), R.ANCHOR_TH,
                         R.COS_TH)


@pytest.mark.parametrize("name", list(R.OCCLUSION_CASES))
def test_occlusion_every_flag(name):
    """every flag equals occlusion_ref: integer coordinates (exact in float32 and float64 alike; ties by the dozen, med == tau
    on the frame that sets tau) and continuous ones (seeds vetted on the reference: no decision within the float32 band); 0, 1,
    2, 3, 64, 65, 129 and T anchors per query; T up to 3072, the largest the 60 KB of LDS hold"""
    case, want, _ = R.occlusion_inputs(name)
    got = device_occlusion(case)
    assert got.dtype == torch.bool and got.shape == (case.N, case.T)
    diff = got.cpu().numpy() != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:8].tolist())


def test_occlusion_refuses_what_the_lds_cannot_hold():
    from dino_tracker_amd import ops
    T = 3073
    z = torch.zeros
    with pytest.raises(RuntimeError, match="libdtk error.*too large"):
        ops.occlusion(z(1, T, 2, device=DEV), torch.tensor([0, 1], dtype=torch.int32, device=DEV),
                      z(1, dtype=torch.int32, device=DEV), z(1, T, 2, device=DEV), torch.ones(1, T, device=DEV), R.ANCHOR_TH,
                      R.COS_TH)


# ---- dtk_traj_cos_sims ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 8, 252, 256, 260, 384, 1024])
@pytest.mark.parametrize("N,T", [(1, 1), (3, 5), (7, 33)])
def test_traj_cos_sims_float64(C, N, T):
    """generic, near-parallel (b = a + 1e-3 noise) and all-zero rows (the eps clamp: 0), tq below 0 and beyond T (clamped).
    Bound: the deterministic float32 worst case of a cosine of magnitude <= 1 -- C roundings in the dot product, C/2 in each of
    the two norms, 8 for the roots, product and quotient: (2C + 8) 2^-24.  One dropped or doubled float4 group moves a cosine by
    about 2/C."""
    from dino_tracker_amd import ops
    rng = np.random.default_rng(100 * C + T)
    bound = (2 * C + 8) * EPS
    for variant in range(2):
        S = rng.standard_normal((N, T, C)).astype(np.float32)
        tq = rng.integers(0, T, N).astype(np.int32)
        q = tq.copy()
        if variant == 0:
            tq[0] = -1
            q[0] = 0
        else:
            tq[-1] = T + 3
            q[-1] = T - 1
        for n in range(N):
            for t in range(1, T, 2):
                if t != q[n]:
                    S[n, t] = S[n, q[n]] + np.float32(1e-3) * rng.standard_normal(C).astype(np.float32)
        if T > 2:
            if variant == 0:
                S[1, (q[1] + 2) % T] = 0  # a zero row against a generic query row
            else:
                S[2, q[2]] = 0  # the query row itself
        want = R.cos_sims_ref(S, tq)
        got = ops.traj_cos_sims(dev(S), dev(tq), N, T)
        assert got.shape == (N, T) and got.dtype == torch.float32
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print(f"cos_sims C={C} N={N} T={T} variant {variant}: max err {err.max():.3e} (bound {bound:.3e})")
        assert err.max() <= bound, (err.max(), bound)
        if T > 2:
            zero = got[1, (q[1] + 2) % T] if variant == 0 else got[2]
            assert (zero == 0).all()


# ---- dtk_sample_points / dtk_sample_grid ---------------------------------------------------------------------------------------
GRIDS = {"19x29": (140, 210), "1x1": (14, 20)}  # video sizes; patch 14, stride 7 (a 1 x 1 grid: any video 14..20 px)


def sample_xy(B, ph, pw, rng):
    """xy = 7 + 7 k / 8: u = k / 8, its fraction and both weights are exact in float32"""
    ku, kv = 8 * (pw - 1), 8 * (ph - 1)
    fixed = [(0, 0), (ku, 0), (0, kv), (ku, kv), (ku - 1, kv - 1), (-20, -3), (ku + 17, kv + 40), (ku + 5, 3), (4, kv + 1)]
    k = np.array(fixed + [(rng.integers(-16, ku + 17), rng.integers(-16, kv + 17)) for _ in range(max(0, B - len(fixed)))])
    if B < len(fixed):
        k = k[3:3 + B]  # the exact last cell first
    return (np.float32(7) + np.float32(7) * k.astype(np.float32) / np.float32(8)).astype(np.float32)


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("C", [4, 252, 256, 260, 1024])
def test_sample_points_float64(C, grid):
    """corners, the exact last cell, out-of-frame points, t_idx below 0 and beyond T, B not a multiple of the four waves of a
    block; scattered through out_row into a larger sentinel-filled buffer.  With exact weights the float32 result is a few
    roundings of the float64 one: 8 * 2^-24 * max|feat|."""
    from dino_tracker_amd import ops
    from dino_tracker_amd._lib import make_geom
    vh, vw = GRIDS[grid]
    rng = np.random.default_rng(C)
    worst = 0.0
    for T in (1, 3):
        g = make_geom(T, C, vh, vw)
        assert f"{g.ph}x{g.pw}" == grid
        feat = rng.standard_normal((T, g.ph * g.pw, C)).astype(np.float32)
        bound = 8 * EPS * float(np.abs(feat).max())
        feat_d = dev(feat)
        for B in (1, 5, 300):
            xy = sample_xy(B, g.ph, g.pw, rng)
            t_idx = rng.integers(0, T, B).astype(np.int32)
            t_idx[0] = T + 1
            if B > 1:
                t_idx[1] = -2
            want = R.sample_points_ref(feat, g.ph, g.pw, 14, 7, xy, t_idx)
            got = ops.sample_points(g, feat_d, dev(xy), dev(t_idx))
            assert got.shape == (B, C)
            err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
            rows = rng.permutation(B + 7)[:B].astype(np.int32)
            out = torch.full((B + 7, C), float(SENTINEL), device=DEV)
            assert ops.sample_points(g, feat_d, dev(xy), dev(t_idx), out=out, out_row=dev(rows)) is out
            out = out.cpu().numpy()
            assert np.array_equal(out[rows], got.cpu().numpy())  # the same values, scattered
            rest = np.setdiff1d(np.arange(B + 7), rows)
            assert (out[rest] == SENTINEL).all()
            worst = max(worst, err / bound)
            assert err <= bound, (T, B, err, bound)
    print(f"sample_points C={C} grid {grid}: max err / bound {worst:.3f}")


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("C", [4, 252, 256, 260, 1024])
def test_sample_grid_float64(C, grid):
    """generic points, coordinates outside [-1, 1] included, integral and fractional t, against the float64 grid_sample;
    the bound is the one tests/test_gpu_bench_path.py::test_sampling_wrappers holds this kernel to, at |feat| <= 4"""
    from dino_tracker_amd import ops
    from dino_tracker_amd._lib import make_geom
    vh, vw = GRIDS[grid]
    rng = np.random.default_rng(7 * C)
    worst = 0.0
    for T in (1, 3):
        g = make_geom(T, C, vh, vw)
        feat = np.clip(rng.standard_normal((T, g.ph * g.pw, C)), -4, 4).astype(np.float32)
        feat_d = dev(feat)
        for B in (1, 5, 300):
            pts = rng.uniform(-1.3, 1.3, (B, 3)).astype(np.float32)
            pts[::2, 2] = rng.integers(0, 3, pts[::2].shape[0]) - 1.0  # integral t: frame 0, 1, 2 of T = 3 exactly
            want = R.sample_grid_ref(feat, g.ph, g.pw, pts)
            got = ops.sample_grid(feat_d, g.ph, g.pw, dev(pts))
            assert got.shape == (B, C)
            err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
            worst = max(worst, err)
            assert err < 2e-5, (T, B, err)
    print(f"sample_grid C={C} grid {grid}: max err {worst:.3e} (bound 2e-5)")


# ---- dtk_pack_features / dtk_unpack_features / dtk_feature_norms ---------------------------------------------------------------
@pytest.mark.parametrize("T,C,HW", [(1, 4, 1), (2, 36, 33), (3, 260, 95), (1, 1024, 31)])
def test_pack_unpack_norms(T, C, HW):
    """both transposes move bits; the norms are within (C/2 + 2) 2^-24 relative of float64 (C/2 roundings of the sum of
    squares -- the root halves the relative error of C of them -- plus the root and the cross-lane sum)"""
    from dino_tracker_amd import ops
    rng = np.random.default_rng(C + HW)
    chw = rng.standard_normal((T, C, 1, HW)).astype(np.float32)
    thwc, norms = ops.pack_features(dev(chw))
    want = np.ascontiguousarray(chw.reshape(T, C, HW).transpose(0, 2, 1))
    assert thwc.shape == (T, HW, C) and np.array_equal(thwc.cpu().numpy().view(np.uint32), want.view(np.uint32))
    back = ops.unpack_features(dev(want), 1, HW)
    assert back.shape == (T, C, 1, HW) and np.array_equal(back.cpu().numpy().view(np.uint32), chw.view(np.uint32))
    ref = np.sqrt((want.astype(np.float64) ** 2).sum(-1))
    bound = (C / 2 + 2) * EPS
    for got in (norms, ops.feature_norms(dev(want))):
        assert got.shape == (T, HW)
        rel = np.abs(got.cpu().numpy().astype(np.float64) - ref) / ref
        print(f"norms T={T} C={C} HW={HW}: max rel err {rel.max():.3e} (bound {bound:.3e})")
        assert rel.max() <= bound, (rel.max(), bound)


# ---- dtk_tapvid_counts ---------------------------------------------------------------------------------------------------------
def device_counts(pred, pocc, gt, gocc, qf, pred_size, gt_size, mode):
    from dino_tracker_amd import tapvid
    counts = tapvid.tapvid_counts(dev(pred), dev(pocc), dev(gt), dev(gocc), dev(qf), pred_size, gt_size, mode)
    assert counts.shape == (18,) and counts.dtype == torch.int64
    return counts.cpu().tolist()


@pytest.mark.parametrize("mode", ["strided", "first"])
@pytest.mark.parametrize("sizes", [((256, 256), (256, 256)), ((512, 128), (128, 512))])
def test_tapvid_counts_on_the_thresholds(mode, sizes):
    """scaled distances of exactly 1, 2, 4, 8 and 16 px along an axis are NOT within (strict <); one float32 ulp below they are.
    The rasters scale by powers of two, so the scaled coordinates are the crafted ones to the bit."""
    pred_size, gt_size = sizes
    rows = []
    for th in (1, 2, 4, 8, 16):
        for axis in (0, 1):
            for below in (False, True):
                for gocc in (False, True):
                    for pocc in (False, True):
                        p = np.array([100, 100], dtype=np.float32)
                        p[axis] = np.float32(100 + th)
                        if below:
                            p[axis] = np.nextafter(p[axis], np.float32(0))
                        rows.append((p, gocc, pocc))
    N = len(rows)
    sp = np.array([256 / pred_size[0], 256 / pred_size[1]], dtype=np.float32)
    sg = np.array([256 / gt_size[0], 256 / gt_size[1]], dtype=np.float32)
    pred = np.zeros((N, 2, 2), dtype=np.float32)
    gt = np.zeros((N, 2, 2), dtype=np.float32)  # frame 0 is the query frame: distance 0, never evaluated
    pred[:, 1] = np.stack([r[0] for r in rows]) / sp
    gt[:, 1] = np.float32(100) / sg
    gocc = np.zeros((N, 2), dtype=bool)
    pocc = np.zeros((N, 2), dtype=bool)
    gocc[:, 1] = [r[1] for r in rows]
    pocc[:, 1] = [r[2] for r in rows]
    qf = np.zeros(N, dtype=np.int32)
    want = R.tapvid_counts_ref(pred, pocc, gt, gocc, qf, pred_size, gt_size, mode)
    # by hand: of the 8 visible points per threshold 2^j (2 axes x 2 predictions x on / below), the 4 on it are within 2^k for
    # j < k, the 4 below it for j <= k
    assert want[0] == N and want[2] == N // 2 and [want[3 + 3 * k] for k in range(5)] == [4 * (2 * k + 1) for k in range(5)]
    assert device_counts(pred, pocc, gt, gocc, qf, pred_size, gt_size, mode) == want


@pytest.mark.parametrize("mode", ["strided", "first"])
@pytest.mark.parametrize("N,T", [(1, 1), (5, 13), (0, 4)])
def test_tapvid_counts_small_and_empty(mode, N, T):
    """one point, 65 points (one wave and one lane of the next), and no query at all: eighteen zeros"""
    rng = np.random.default_rng(N * T)
    gt = (rng.random((N, T, 2)) * [1280, 720]).astype(np.float32)
    pred = (gt * [854 / 1280, 476 / 720] + rng.normal(0, 1, (N, T, 2)) * rng.choice([1, 4, 16, 60], (N, T, 1))).astype(np.float32)
    gocc, pocc = rng.random((N, T)) < 0.3, rng.random((N, T)) < 0.3
    qf = (rng.integers(0, T, N) if T > 1 else np.full(N, -1)).astype(np.int32)  # T = 1: the one frame is evaluated
    want = R.tapvid_counts_ref(pred, pocc, gt, gocc, qf, (854, 476), (1280, 720), mode)
    if N == 0:
        assert want == [0] * 18
    elif T == 1:
        assert want[0] == 1
    assert device_counts(pred, pocc, gt, gocc, qf, (854, 476), (1280, 720), mode) == want
