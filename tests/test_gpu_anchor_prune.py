"""GPU: the pruned anchor stage (dtk_build_anchor_sources_needed / dtk_occlusion_needed, csrc/anchors.hip) against the plain
references of tests/anchor_prune_ref.py and against the full stage, exactly: the builder at the shapes and patterns of
tests/test_gpu_anchor_stage.py, the flags at every OCCLUSION_CASES input set with NaN outside the needed cells of green, and
ModelInference.infer end to end against its own full_anchor_stage and the oracle at thresholds placed between the cosines."""
import numpy as np
import pytest
import torch

import anchor_prune_ref as P
import anchor_stage_ref as R
from dino_tracker_amd import ops, synth
from oracle import ref_algo as A
from test_gpu_anchor_stage import PATTERNS, SENTINEL, SOURCE_SHAPES, cs_pattern, dev, sentinel_buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATH, CTH = R.ANCHOR_TH, R.COS_TH
PX_TOL = 1e-3


# ---- dtk_build_anchor_sources_needed -------------------------------------------------------------------------------------------
def check_needed_sources(buf, want, N, T, untouched_is_sentinel=True):
    P_, M = int(want.counts[0]), int(want.counts[1])
    assert buf.counts.cpu().numpy().tolist() == want.counts.tolist()
    assert np.array_equal(buf.n_anchors.cpu().numpy(), want.n_anchors)
    assert buf.pair_off.numel() == N + 1 and np.array_equal(buf.pair_off.cpu().numpy(), want.pair_off)
    assert np.array_equal(buf.pair_frame[:P_].cpu().numpy(), want.pair_frame)
    for name in ("src_row", "tgt", "out_idx"):
        assert np.array_equal(getattr(buf, name)[:M].cpu().numpy(), getattr(want, name)), name
    if untouched_is_sentinel:
        assert (buf.pair_frame[P_:] == SENTINEL).all()
        for name in ("src_row", "tgt", "out_idx"):
            assert getattr(buf, name).numel() == N * T * T and (getattr(buf, name)[M:] == SENTINEL).all(), name


def query_kinds(want):
    has_anchor = want.n_anchors > 0
    found = {"open": want.masks.open.any(), "closed": (has_anchor & ~want.masks.open).any(), "none": (~has_anchor).any(),
             "dropped": (~want.masks.needed[want.masks.open]).any()}
    return {k for k, v in found.items() if v}


@pytest.mark.parametrize("N,T", SOURCE_SHAPES)
def test_build_needed_sources_exact(N, T):
    """every output equals needed_sources_ref on its valid prefix, counts[0..3] exactly, nothing behind the prefix is written, and
    the pair bookkeeping is what dtk_build_anchor_sources writes for the same cs"""
    kinds = set()
    for i, pattern in enumerate(PATTERNS):
        cs = cs_pattern(pattern, N, T, 1000 * N + 10 * T + i)
        want = P.needed_sources_ref(cs, ATH, CTH)
        kinds |= query_kinds(want)
        buf = sentinel_buffers(N, T)
        assert ops.build_anchor_sources_needed(dev(cs), ATH, CTH, buf) is buf
        check_needed_sources(buf, want, N, T)
        full = ops.build_anchor_sources(dev(cs), ATH, sentinel_buffers(N, T))
        for name in ("n_anchors", "pair_off", "pair_frame"):
            assert torch.equal(getattr(buf, name), getattr(full, name)), name   # sentinel tails included
        assert buf.counts[0] == full.counts[0] and buf.counts[2] == full.counts[2]
    if N * T >= 35:
        assert kinds == {"open", "closed", "none", "dropped"}, kinds   # (asserted on the references alone)


def test_build_needed_sources_reuses_its_buffers():
    """a dense call (every query open, every column needed) followed by a sparse one into the same buffers"""
    N, T = 257, 16
    dense = np.full((N, T), 0.95, dtype=np.float32)
    dense[:, 3] = 0.65   # one undecided frame per query: all open, all columns needed
    sparse = cs_pattern("mixed", N, T, 2)
    buf = sentinel_buffers(N, T)
    ops.build_anchor_sources_needed(dev(dense), ATH, CTH, buf)
    want = P.needed_sources_ref(dense, ATH, CTH)
    assert want.counts.tolist() == [N * (T - 1), N * (T - 1) * T, 0, N]
    check_needed_sources(buf, want, N, T)
    assert ops.build_anchor_sources_needed(dev(sparse), ATH, CTH, buf) is buf
    want = P.needed_sources_ref(sparse, ATH, CTH)
    assert 0 < want.counts[1] < want.counts[0] * T and want.counts[2] > 0 and 0 < want.counts[3] < N
    check_needed_sources(buf, want, N, T, untouched_is_sentinel=False)


# ---- dtk_occlusion_needed ------------------------------------------------------------------------------------------------------
def device_flags(case, green, needed_only):
    return ops.occlusion(dev(green), dev(case.pair_off), dev(case.pair_frame), dev(case.traj), dev(case.cs), ATH, CTH, needed_only)


@pytest.mark.parametrize("name", list(R.OCCLUSION_CASES))
def test_occlusion_needed_every_flag(name):
    """green NaN outside the needed cells: the flags are those of dtk_occlusion on the full green (and of occlusion_ref)"""
    case, want, _ = R.occlusion_inputs(name)
    full = device_flags(case, case.green, False)
    got = device_flags(case, P.prune_green(case.green, case.cs, case.pair_off, ATH, CTH), True)
    assert got.dtype == torch.bool and got.shape == (case.N, case.T)
    assert torch.equal(got, full), int((got != full).sum())
    assert np.array_equal(got.cpu().numpy(), want)


def test_occlusion_needed_refuses_what_the_lds_cannot_hold():
    T = 3073
    z = torch.zeros
    with pytest.raises(RuntimeError, match="libdtk error.*too large"):
        ops.occlusion(z(1, T, 2, device=DEV), torch.tensor([0, 1], dtype=torch.int32, device=DEV), z(1, dtype=torch.int32, device=DEV),
                      z(1, T, 2, device=DEV), torch.ones(1, T, device=DEV), ATH, CTH, True)


# ---- ModelInference.infer ------------------------------------------------------------------------------------------------------
def thresholds_between(cs):
    """(anchor_th, cos_th), each midway between two adjacent distinct cosines at least 1e-3 apart (so that the oracle's cosines,
    within 1e-5 of the device's, fall on the same sides), such that the case holds an all-anchor query, an open query that drops a
    low column and an open query count below N; the highest such pair, or None"""
    v = np.unique(cs[np.isfinite(cs)].astype(np.float64))
    mids = [(a + b) / 2 for a, b in zip(v[:-1], v[1:]) if b - a >= 1e-3][::-1]
    for i, ath in enumerate(mids):
        for cth in mids[i + 1:]:
            m = P.masks(cs, ath, cth)
            all_anchor = m.anchor.all(axis=1)
            dropping = m.open & (~m.needed).any(axis=1)
            if all_anchor.any() and dropping.any() and (~m.open).any():
                return float(ath), float(cth)
    return None


E2E = {"67x121": (476, 854, lambda H, W: torch.cat([synth.grid_queries(4, 3, H, W, 0), synth.grid_queries(2, 2, H, W, 3)]), 41),
       "35x35": (256, 256, lambda H, W: synth.grid_queries(4, 3, H, W, 1), 70)}


@pytest.mark.parametrize("method", [ops.TRACK_EXACT, ops.TRACK_MFMA], ids=["exact", "mfma"])
@pytest.mark.parametrize("grid", list(E2E))
def test_infer_pruned_equals_full_and_oracle(grid, method):
    """infer with the pruned stage: positions and flags torch.equal to full_anchor_stage = True, flags equal to the oracle, the
    anchor-stage dtk_track call ran exactly the reference's needed count, last_counts[0] still counts every pair; then thresholds
    (0.5, 0.5): no anchor source at all"""
    from gpu_util import make_inference, make_tracker
    H, W, make_queries, seed = E2E[grid]
    T, C = 6, 384
    ph, pw = A.feature_grid(H, W)
    feats = synth.synth_features(T, C, ph, pw, seed=seed)
    head = synth.synth_head_weights(3)
    queries = make_queries(H, W)
    N = queries.shape[0]
    trk = make_tracker(torch.zeros(T, 3, H, W), feats, head, method=method)
    mi = make_inference(trk, H, W, T)
    cs = mi.compute_trajectory_cos_sims(mi.compute_trajectories(queries.cuda()), queries.cuda()).cpu().numpy()
    picked = thresholds_between(cs)
    assert picked is not None, np.sort(cs.ravel())
    ath, cth = picked
    m = P.masks(cs, ath, cth)
    n_open = int(m.open.sum())
    assert m.anchor.all(axis=1).any() and (m.open & (~m.needed).any(axis=1)).any() and 0 < n_open < N and m.anchor.any(axis=1).all()
    assert np.abs(cs - np.float32(ath)).min() >= 4e-4 and np.abs(cs - np.float32(cth)).min() >= 4e-4
    want_sources = P.needed_count(cs, ath, cth)[0]
    print(f"{grid} {method}: thresholds {ath:.4f} / {cth:.4f}, {n_open} of {N} queries open, {want_sources} of "
          f"{int(m.anchor.sum()) * T} anchor sources needed")

    mi = make_inference(trk, H, W, T, ath, cth)
    mi.full_anchor_stage = False   # (whatever the environment chose: both are run)
    traj, occ = mi.infer(queries.cuda())
    assert trk.last_track_stats["sources"] == want_sources
    assert mi.last_counts.tolist() == [int(m.anchor.sum()), want_sources, 0, n_open]
    mi.full_anchor_stage = True
    traj_full, occ_full = mi.infer(queries.cuda())
    assert trk.last_track_stats["sources"] == int(m.anchor.sum()) * T and int(mi.last_counts[0]) == int(m.anchor.sum())
    assert torch.equal(traj, traj_full) and torch.equal(occ, occ_full)
    rt, ro, rcs, _ = A.infer(feats, queries, head, H, W, anchor_th=ath, cos_th=cth, return_aux=True)
    assert (traj.cpu() - rt).abs().max() < PX_TOL and np.abs(cs - rcs.numpy()).max() < 1e-5
    assert torch.equal(occ.cpu(), ro), int((occ.cpu() != ro).sum())

    # no band between the thresholds: every query closed, no anchor-stage dtk_track call, flags = low
    mi = make_inference(trk, H, W, T, 0.5, 0.5)
    mi.full_anchor_stage = False
    _, occ = mi.infer(queries.cuda())
    assert trk.last_track_stats == {"sources": 0, "whole_map_tier": 0, "exact_tier": 0, "syncs": 0}
    assert mi.last_counts.tolist() == [int((cs >= np.float32(0.5)).sum()), 0, 0, 0]
    ro = A.infer(feats, queries, head, H, W, anchor_th=0.5, cos_th=0.5)[1]
    assert torch.equal(occ.cpu(), ro), int((occ.cpu() != ro).sum())
