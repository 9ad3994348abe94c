"""CPU: the pruned anchor stage is exact.  For every input set of tests/anchor_stage_ref.py the flags computed from the needed
cells of green alone (every other cell NaN) equal occlusion_ref on the full green -- at the reference's thresholds, at the class
defaults (0.5, 0.5: no band), at an inverted pair and with NaN cosines -- and the sets hold every kind of query.  References
only; the device is held to them by tests/test_gpu_anchor_prune.py."""
import numpy as np
import pytest

import anchor_prune_ref as P
import anchor_stage_ref as R

NOT_3072 = [name for name in R.OCCLUSION_CASES if not name.startswith("T3072")]


def flags_full(case, anchor_th, cos_th):
    return R.occlusion_ref(case.green, case.pair_off, case.pair_frame, case.traj, case.cs, anchor_th, cos_th)[0]


@pytest.mark.parametrize("with_nan", [False, True], ids=["finite", "nan_cs"])
@pytest.mark.parametrize("anchor_th,cos_th", P.THRESHOLD_PAIRS)
@pytest.mark.parametrize("name", list(R.OCCLUSION_CASES))
def test_pruned_flags_equal_full_flags(name, anchor_th, cos_th, with_nan):
    case = P.case_at(name, anchor_th, with_nan)
    if anchor_th == R.ANCHOR_TH and cos_th == R.COS_TH and not with_nan:
        want = R.occlusion_inputs(name)[1]   # the shared reference
    else:
        want = flags_full(case, anchor_th, cos_th)
    pruned = P.prune_green(case.green, case.cs, case.pair_off, anchor_th, cos_th)
    # (pruned_occlusion_ref asserts that no NaN reaches its distances: it reads the needed cells only)
    got = P.pruned_occlusion_ref(pruned, case.pair_off, case.pair_frame, case.traj, case.cs, anchor_th, cos_th)
    diff = got != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:8].tolist())
    # the issue's own check: huge values outside the needed set do not move a flag of the FULL reference either
    huge = P.prune_green(case.green, case.cs, case.pair_off, anchor_th, cos_th, fill=1e30)
    assert np.array_equal(R.occlusion_ref(huge, case.pair_off, case.pair_frame, case.traj, case.cs, anchor_th, cos_th)[0], want)
    if not with_nan and anchor_th <= cos_th:
        assert not P.masks(case.cs, anchor_th, cos_th).open.any()   # no band between the thresholds: nothing to track


def test_input_sets_hold_every_kind_of_query():
    """at (0.7, 0.6), over all sets but T3072_*: 518 of 700 queries open, 227 288 of 764 026 sources needed; closed queries with
    anchors and queries without anchors both occur, and open queries drop columns (low and not an anchor)"""
    queries = opened = closed_with_anchors = without_anchors = needed = full = dropped_columns = 0
    for name in NOT_3072:
        case = R.occlusion_inputs(name)[0]
        m = P.masks(case.cs, R.ANCHOR_TH, R.COS_TH)
        has_anchor = m.anchor.any(axis=1)
        queries += case.N
        opened += int(m.open.sum())
        closed_with_anchors += int((has_anchor & ~m.open).sum())
        without_anchors += int((~has_anchor).sum())
        needed += P.needed_count(case.cs, R.ANCHOR_TH, R.COS_TH)[0]
        full += int(case.pair_off[-1]) * case.T
        dropped_columns += int((~m.needed[m.open]).sum())
    assert (queries, opened) == (700, 518)
    assert (needed, full) == (227288, 764026)
    assert closed_with_anchors > 0 and without_anchors > 0 and dropped_columns > 0
    assert opened + closed_with_anchors + without_anchors == queries


@pytest.mark.parametrize("anchor_th,cos_th", P.THRESHOLD_PAIRS)
def test_needed_sources_ref_against_the_full_list(anchor_th, cos_th):
    """the needed list is the full list of anchor_sources_ref with the entries of closed queries and of non-needed columns taken
    out, order kept; its pair bookkeeping is the full one's"""
    rng = np.random.default_rng(5)
    cs = rng.uniform(0.4, 0.9, (37, 9)).astype(np.float32)
    cs[rng.random(cs.shape) < 0.1] = np.nan
    cs[:5] = 0.95            # closed: all anchors
    cs[5:8] = 0.2            # no anchors
    cs[8, :] = 0.65          # undecided frames but no anchor: closed
    full = R.anchor_sources_ref(cs, anchor_th)
    got = P.needed_sources_ref(cs, anchor_th, cos_th)
    for name in ("n_anchors", "pair_off", "pair_frame"):
        assert np.array_equal(getattr(got, name), getattr(full, name)), name
    assert got.counts[0] == full.counts[0] and got.counts[2] == full.counts[2]
    T = cs.shape[1]
    n_of, t_of = full.src_row // T, full.src_row % T
    keep = got.masks.open[n_of] & got.masks.needed[n_of, t_of]
    for name in ("src_row", "tgt", "out_idx"):
        assert np.array_equal(getattr(got, name), getattr(full, name)[keep]), name
    assert (got.counts[1], got.counts[3]) == P.needed_count(cs, anchor_th, cos_th) == (int(keep.sum()), int(got.masks.open.sum()))
    assert got.counts[3] > 0 or anchor_th <= cos_th and not np.isnan(cs).any()
