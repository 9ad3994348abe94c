"""Plain CPU references for the pruned anchor stage (dtk_build_anchor_sources_needed / dtk_occlusion_needed in csrc/anchors.hip),
written from the definitions of include/dtk.h.  Both cs comparisons are made on the float32 values:

    anchor(n,t) = cs >= anchor_th      low(n,t) = cs < cos_th      undecided = !anchor and !low (a NaN cs is undecided)
    needed(n,t) = anchor or undecided  query n open = at least one anchor and at least one undecided frame

The input sets come from tests/anchor_stage_ref.py (imported, not edited).  Nothing here touches the library."""
from types import SimpleNamespace

import numpy as np

import anchor_stage_ref as R

F32 = np.float32
THRESHOLD_PAIRS = [(0.7, 0.6), (0.5, 0.5), (0.6, 0.7)]   # the reference's, the class defaults (no band), an inverted pair


def masks(cs, anchor_th, cos_th):
    """cs [N,T] -> anchor, low, undecided, needed [N,T] bool and open [N] bool"""
    cs = np.asarray(cs, dtype=F32)
    anchor = cs >= F32(anchor_th)
    low = cs < F32(cos_th)
    undecided = ~anchor & ~low
    needed = anchor | undecided
    is_open = anchor.any(axis=1) & undecided.any(axis=1)
    return SimpleNamespace(anchor=anchor, low=low, undecided=undecided, needed=needed, open=is_open)


def pair_structure(cs, anchor_th):
    """n_anchors [N], pair_off [N+1], pair_frame [P] of anchor_sources_ref, without its source lists (cheap at T = 3072)"""
    anchor = np.asarray(cs, dtype=F32) >= F32(anchor_th)
    n_anchors = anchor.sum(axis=1).astype(np.int32)
    pair_off = np.zeros(anchor.shape[0] + 1, dtype=np.int32)
    pair_off[1:] = np.cumsum(n_anchors)
    pair_frame = np.nonzero(anchor)[1].astype(np.int32)   # row-major: n-major, frames ascending
    return n_anchors, pair_off, pair_frame


def needed_sources_ref(cs, anchor_th, cos_th):
    """The outputs of dtk_build_anchor_sources_needed: the pair bookkeeping of anchor_sources_ref and the source list of
    (open n, anchor a of n, needed column t of n), sorted by a, within a by n, within a pair by t; entry = (n*T + t, a, p*T + t).
    counts = [pairs, emitted sources, queries without anchors, open queries]."""
    cs = np.asarray(cs, dtype=F32)
    N, T = cs.shape
    m = masks(cs, anchor_th, cos_th)
    n_anchors, pair_off, pair_frame = pair_structure(cs, anchor_th)
    src_row, tgt, out_idx = [], [], []
    for a in range(T):
        for n in range(N):
            if not (m.anchor[n, a] and m.open[n]):
                continue
            p = int(pair_off[n]) + int(m.anchor[n, :a].sum())
            for t in range(T):
                if m.needed[n, t]:
                    src_row.append(n * T + t)
                    tgt.append(a)
                    out_idx.append(p * T + t)
    counts = np.array([pair_off[N], len(src_row), int((n_anchors == 0).sum()), int(m.open.sum())], dtype=np.int32)
    i32 = lambda v: np.array(v, dtype=np.int32)
    return SimpleNamespace(n_anchors=n_anchors, pair_off=pair_off, pair_frame=pair_frame, counts=counts, src_row=i32(src_row),
                           tgt=i32(tgt), out_idx=i32(out_idx), masks=m)


def needed_count(cs, anchor_th, cos_th):
    """(emitted sources, open queries) without the lists: every anchor pair of an open query emits its needed columns"""
    m = masks(cs, anchor_th, cos_th)
    per_query = m.anchor.sum(axis=1).astype(np.int64) * m.needed.sum(axis=1)
    return int(per_query[m.open].sum()), int(m.open.sum())


def green_needed_mask(cs, pair_off, anchor_th, cos_th):
    """[P,T] bool: the cells of green the pruned stage writes and reads"""
    m = masks(cs, anchor_th, cos_th)
    P = int(pair_off[-1])
    keep = np.zeros((P, cs.shape[1]), dtype=bool)
    for n in range(cs.shape[0]):
        if m.open[n]:
            keep[int(pair_off[n]):int(pair_off[n + 1])] = m.needed[n]
    return keep


def prune_green(green, cs, pair_off, anchor_th, cos_th, fill=np.nan):
    """a copy of green [P,T,2] with `fill` in every cell outside the needed set"""
    out = np.array(green, dtype=F32, copy=True)
    out[~green_needed_mask(cs, pair_off, anchor_th, cos_th)] = fill
    return out


def pruned_occlusion_ref(green, pair_off, pair_frame, traj, cs, anchor_th, cos_th):
    """occ [N,T] bool from the needed cells of green alone (occlusion_ref's float64 arithmetic there): a query without anchors is
    all ones, a closed query low(n,t); an open query takes tau from its anchor columns, (med > tau) | low at its needed columns
    and low at the others."""
    green = np.asarray(green, dtype=np.float64)
    traj = np.asarray(traj, dtype=np.float64)
    cs = np.asarray(cs, dtype=F32)
    N, T = cs.shape
    m = masks(cs, anchor_th, cos_th)
    occ = m.low.copy()
    for n in range(N):
        p0, p1 = int(pair_off[n]), int(pair_off[n + 1])
        A = p1 - p0
        if A <= 0:
            occ[n] = True
            continue
        if not m.open[n]:
            continue
        cols = np.nonzero(m.needed[n])[0]
        frames = np.asarray(pair_frame[p0:p1], dtype=np.int64)
        diff = green[p0:p1][:, cols] - traj[n][frames][:, None, :]   # [A, needed, 2]
        d = np.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1])
        assert np.isfinite(d).all(), "a cell outside the needed set (NaN in the tests) was read"
        med = np.sort(d, axis=0)[(A - 1) // 2]
        tau = med[m.anchor[n][cols]].max()
        occ[n, cols] = (med > tau) | m.low[n, cols]
    return occ


# --------------------------------------------------------------------------------------------------------------
# input sets at other thresholds / with NaN cosines: the cs of an OCCLUSION_CASES entry, its pairs rebuilt for the threshold
# --------------------------------------------------------------------------------------------------------------
def nan_cs(cs, seed):
    """about one cosine in eight replaced by NaN (never an anchor, never low: undecided)"""
    out = np.array(cs, dtype=F32, copy=True)
    out[np.random.default_rng(seed).random(out.shape) < 0.125] = np.nan
    return out


def case_at(name, anchor_th, with_nan=False):
    """OCCLUSION_CASES[name] with pair_off / pair_frame / green rebuilt for anchor_th (and NaN cosines): the case of
    anchor_stage_ref itself where nothing changes"""
    base, _, _ = R.occlusion_inputs(name)
    if anchor_th == R.ANCHOR_TH and not with_nan:
        return base
    cs = nan_cs(base.cs, 77 + base.T) if with_nan else base.cs
    _, pair_off, pair_frame = pair_structure(cs, anchor_th)
    P = int(pair_off[-1])
    rng = np.random.default_rng(9000 + base.T)
    if base.kind == "int":
        green = rng.integers(0, 64, (P, base.T, 2)).astype(F32)
    else:
        green = (rng.random((P, base.T, 2)) * np.array([854.0, 476.0])).astype(F32)
    return SimpleNamespace(T=base.T, N=base.N, kind=base.kind, cs=cs, pair_off=pair_off, pair_frame=pair_frame, green=green,
                           traj=base.traj)
