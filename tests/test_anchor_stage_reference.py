"""CPU: the plain references of tests/anchor_stage_ref.py against what the project already trusts (oracle/ref_algo.py, itself
pinned to the reference by tests/test_oracle_vs_reference.py), and the conditions under which the input sets of
tests/test_gpu_anchor_stage.py may be compared flag for flag, asserted on the references alone."""
import numpy as np
import pytest
import torch

import anchor_stage_ref as R
from oracle import ref_algo as A


def _random_cs(n, t, seed, every_row_anchored=True):
    rng = np.random.default_rng(seed)
    cs = rng.uniform(0.3, 1.0, (n, t)).astype(np.float32)
    if every_row_anchored:
        cs[np.arange(n), rng.integers(0, t, n)] = 0.9
    return cs, rng


@pytest.mark.parametrize("kind", ["int", "cont"])
@pytest.mark.parametrize("n,t", [(1, 1), (4, 2), (6, 9), (3, 70)])
def test_occlusion_ref_equals_oracle(kind, n, t):
    """occlusion_ref == oracle.ref_algo.occlusion_for_query (models/model_inference.py:169-177) for every query with anchors;
    the oracle runs on the same float64 operands, so that near-ties cannot separate the two"""
    cs, rng = _random_cs(n, t, 10 * n + t, every_row_anchored=False)
    cs[0, 0] = np.float32(R.ANCHOR_TH)  # on the threshold: an anchor
    src = R.anchor_sources_ref(cs, R.ANCHOR_TH)
    P = int(src.counts[0])
    if kind == "int":
        green, traj = rng.integers(0, 64, (P, t, 2)).astype(np.float32), rng.integers(0, 64, (n, t, 2)).astype(np.float32)
    else:
        green, traj = (rng.random((P, t, 2)) * 400).astype(np.float32), (rng.random((n, t, 2)) * 400).astype(np.float32)
    occ, margin = R.occlusion_ref(green, src.pair_off, src.pair_frame, traj, cs, R.ANCHOR_TH, R.COS_TH)
    checked = 0
    for i in range(n):
        p0, p1 = int(src.pair_off[i]), int(src.pair_off[i + 1])
        if p1 == p0:
            assert occ[i].all() and np.isinf(margin[i]).all()
            continue
        want = A.occlusion_for_query(torch.from_numpy(green[p0:p1]).double(), torch.from_numpy(traj[i]).double(),
                                     torch.from_numpy(cs[i]), R.ANCHOR_TH, R.COS_TH)
        assert np.array_equal(occ[i], want.numpy()), i
        m_med, _ = A.occlusion_margins(torch.from_numpy(green[p0:p1]).double(), torch.from_numpy(traj[i]).double(),
                                       torch.from_numpy(cs[i]), R.ANCHOR_TH, R.COS_TH)
        assert np.allclose(margin[i], m_med.numpy(), rtol=0, atol=1e-9)
        checked += 1
    assert checked


def test_occlusion_ref_semantics_by_hand():
    """lower median of an even count, med == tau reads as visible, cs == cos_th is visible, no anchor -> all ones"""
    # query 0: T = 6, anchors at frames 0 and 2 (cs == th counts); traj at the origin, greens on the x axis
    th, cos = np.float32(R.ANCHOR_TH), np.float32(R.COS_TH)
    cs = np.array([[th, cos, 0.9, np.nextafter(cos, np.float32(0)), 0.65, 0.65], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]],
                  dtype=np.float32)
    src = R.anchor_sources_ref(cs, R.ANCHOR_TH)
    assert list(src.n_anchors) == [2, 0] and list(src.pair_frame) == [0, 2] and list(src.counts) == [2, 12, 1]
    traj = np.zeros((2, 6, 2), dtype=np.float32)
    green = np.zeros((2, 6, 2), dtype=np.float32)
    green[0, :, 0] = [1, 2, 3, 1, 3, 5]   # distances of anchor pair 0 per frame
    green[1, :, 0] = [2, 1, 3, 2, 4, 4]   # ... of anchor pair 1: lower medians 1 1 3 1 3 4, tau = max(med[0], med[2]) = 3
    occ, margin = R.occlusion_ref(green, src.pair_off, src.pair_frame, traj, cs, R.ANCHOR_TH, R.COS_TH)
    # frame 1: cs == cos_th visible; 2: med == tau visible; 3: cs one ulp below cos_th; 4: the LOWER median 3 == tau (the
    # upper one, 4, would be occluded); 5: med > tau
    assert occ[0].tolist() == [False, False, False, True, False, True]
    assert margin[0].tolist() == [2, 2, 0, 2, 0, 1]
    assert occ[1].all()


@pytest.mark.parametrize("n,t", [(1, 1), (5, 7), (3, 40)])
def test_anchor_sources_regroup_to_the_oracle_lists(n, t):
    """src_row / tgt regrouped by out_idx are a_row / a_tgt as oracle.ref_algo.infer builds them: the property
    ModelInference._anchor_stage relies on when it scatters the anchor trajectories to pair-major order"""
    cs, _ = _random_cs(n, t, 100 * n + t)
    src = R.anchor_sources_ref(cs, R.ANCHOR_TH)
    # the oracle's construction, verbatim
    cst = torch.from_numpy(cs)
    anchors_of = [torch.nonzero(cst[i] >= R.ANCHOR_TH)[:, 0] for i in range(n)]
    t_ar = torch.arange(t)
    a_row = torch.cat([(i * t + t_ar)[None].expand(a.numel(), -1).reshape(-1) for i, a in enumerate(anchors_of)])
    a_tgt = torch.cat([a[:, None].expand(-1, t).reshape(-1) for a in anchors_of])
    M = int(src.counts[1])
    assert M == a_row.numel() == src.src_row.size
    assert sorted(src.out_idx.tolist()) == list(range(M))  # a permutation of the pair-major rows
    back = np.empty(M, dtype=np.int64)
    back[src.out_idx] = np.arange(M)
    assert np.array_equal(src.src_row[back], a_row.numpy())
    assert np.array_equal(src.tgt[back], a_tgt.numpy())
    assert np.array_equal(src.pair_frame, torch.cat(anchors_of).numpy())
    # sorted by anchor frame, within a frame by query
    key = src.tgt.astype(np.int64)[::t] * n + src.src_row[::t] // t
    assert (np.diff(key) > 0).all()


def test_anchor_sources_nan_and_threshold():
    cs = np.array([[np.nan, 0.7, 0.69999], [np.nan, np.nan, 0.1]], dtype=np.float32)
    src = R.anchor_sources_ref(cs, 0.7)
    assert list(src.n_anchors) == [1, 0] and list(src.pair_off) == [0, 1, 1] and list(src.counts) == [1, 3, 1]
    assert list(src.src_row) == [0, 1, 2] and list(src.tgt) == [1, 1, 1] and list(src.out_idx) == [0, 1, 2]


@pytest.mark.parametrize("mode", ["strided", "first"])
def test_tapvid_counts_ref_folds_to_the_oracle_metrics(mode):
    rng = np.random.default_rng(5)
    n, t = 23, 17
    gt = (rng.random((n, t, 2)) * [1280, 720]).astype(np.float32)
    pred = (gt * [854 / 1280, 476 / 720] + rng.normal(0, 1, (n, t, 2)) * rng.choice([1, 4, 16, 60], (n, t, 1))).astype(np.float32)
    gocc, pocc = rng.random((n, t)) < 0.3, rng.random((n, t)) < 0.3
    qf = rng.integers(0, t - 1, n)
    counts = R.tapvid_counts_ref(pred, pocc, gt, gocc, qf, (854, 476), (1280, 720), mode)
    got = R.metrics_from_counts_ref(counts)
    want = A.tapvid_metrics(qf, gocc, gt, pocc, pred, (854, 476), (1280, 720), mode)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12), k
    assert 0 < counts[3] < counts[15] < counts[2] < counts[0]  # the thresholds separate something


# ---- conditions on the input sets of tests/test_gpu_anchor_stage.py -------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.OCCLUSION_CASES))
def test_input_set_conditions(name):
    """What lets the GPU test compare EVERY flag of a float32 kernel with a float64 reference.

    int sets: squared distances are integers <= 8192, exact in both precisions; distinct distances differ by at least
    sqrt(8192) - sqrt(8191) = 5.5e-3 px, so no decision may have 0 < |med - tau| < 5e-3 (exact ties are wanted).
    cont sets: no decision closer than 1e-4 px (the issue's figure), and no closer than the float32 evaluation of two
    distances can move them: each is 2.5 roundings of 2^-24 relative (the subtraction, square, sum and half the root) of at
    most 978 px.  The one exception is by construction, not by precision: on an anchor frame med <= tau holds in ANY arithmetic
    (tau is the maximum over exactly those frames), so such a frame is visible in the kernel and in the reference whatever its
    margin; the frame that sets tau has margin 0."""
    case, occ, margin = R.occlusion_inputs(name)
    T, _, _, _ = R.OCCLUSION_CASES[name]
    assert case.cs.shape == (case.N, T) and case.green.shape == (int(case.pair_off[-1]), T, 2)
    assert not np.isnan(case.green).any() and not np.isnan(case.traj).any() and not np.isnan(case.cs).any()
    has = np.array(case.counts) > 0
    m = margin[has]
    anchor = (case.cs >= np.float32(R.ANCHOR_TH))[has]
    assert (m[anchor] >= 0).all() and not occ[has][anchor & (case.cs[has] >= np.float32(R.COS_TH))].any()
    if case.kind == "int":
        assert not ((m > 0) & (m < 5e-3)).any(), m[(m > 0)].min()
        assert (m[anchor] == 0).sum() >= has.sum()  # every anchored query has its med == tau frame
        assert np.abs(case.green).max() < 64 and (case.green == np.round(case.green)).all()
    else:
        fp32_band = 2 * 2.5 * 2.0 ** -24 * np.hypot(854, 476)
        assert fp32_band < 3e-4
        free = m[~anchor]
        if free.size:
            assert free.min() >= max(1e-4, fp32_band), free.min()
    # the case holds what it was built to hold
    assert sorted(set(case.counts)) == sorted(set(R.anchor_counts_for(T))) or name.startswith(("N300", "T3072"))
    if 5 <= T <= 300:  # both outcomes occur
        assert occ[has].any() and not occ[has].all()


def test_occlusion_cases_cover_the_paths():
    """anchors per query 0, 1, 2, 3, 64, 65, 129 and T; T beyond one 256-thread stride; both thresholds hit exactly"""
    seen = set()
    for name in R.OCCLUSION_CASES:
        case, _, _ = R.occlusion_inputs(name)
        seen |= set(int(c) for c in case.counts)
        if case.T >= 3:
            assert (case.cs == np.float32(R.ANCHOR_TH)).any() and (case.cs == np.float32(R.COS_TH)).any(), name
    assert {0, 1, 2, 3, 64, 65, 129, 130, 257, 300} <= seen


# ---- the float64 sampling and cosine references against each other and against torch --------------------------------------------
def test_cos_sims_ref_is_cosine_similarity():
    import torch.nn.functional as F
    rng = np.random.default_rng(3)
    S = rng.standard_normal((4, 6, 20)).astype(np.float32)
    S[1, 2] = 0
    tq = np.array([-1, 0, 9, 3])
    want = F.cosine_similarity(torch.from_numpy(S).double()[torch.arange(4), torch.tensor([0, 0, 5, 3])][:, None],
                               torch.from_numpy(S).double(), dim=-1)
    got = R.cos_sims_ref(S, tq)
    assert np.abs(got - want.numpy()).max() < 1e-14 and (got[1, 2] == 0) and np.allclose(got[[0, 1, 2, 3], [0, 0, 5, 3]], 1)


@pytest.mark.parametrize("vh,vw", [(140, 210), (14, 20)])
def test_sampling_refs_agree(vh, vw):
    """sample_points_ref (pixel coordinates, the clamping of core.hip restated) == oracle.sample_bilinear in float64 ==
    sample_grid_ref (float64 grid_sample) at the same points in grid coordinates, border clamp included"""
    rng = np.random.default_rng(vh)
    T, C = 3, 8
    ph, pw = A.feature_grid(vh, vw)
    feat = rng.standard_normal((T, ph * pw, C)).astype(np.float32)
    xy = (rng.random((200, 2)) * [vw + 40, vh + 40] - 20).astype(np.float32)
    xy[:4] = [[7, 7], [7 * pw, 7 * ph], [7 * pw, 7], [-3, 7 * ph + 9]]
    t = rng.integers(0, T, 200)
    got = R.sample_points_ref(feat, ph, pw, 14, 7, xy, t)
    chw = torch.from_numpy(feat).double().reshape(T, ph, pw, C).permute(0, 3, 1, 2)
    want = A.sample_bilinear(chw, torch.from_numpy(xy).double(), torch.from_numpy(t), vh, vw).numpy()
    assert np.abs(got - want).max() < 1e-12
    u = (xy.astype(np.float64) - 7) / 7
    one = lambda x, size: np.zeros_like(x) if size == 1 else x / (size - 1) * 2 - 1  # noqa: E731
    pts = np.stack([one(u[:, 0], pw), one(u[:, 1], ph), t / (T - 1) * 2 - 1], axis=1)
    assert np.abs(R.sample_grid_ref(feat, ph, pw, pts) - got).max() < 1e-12
    # t beyond the ends is clamped
    at = lambda tt: R.sample_points_ref(feat, ph, pw, 14, 7, xy, tt)  # noqa: E731
    assert np.array_equal(at(t + T), at(t * 0 + T - 1)) and np.array_equal(at(t - T), at(t * 0))
