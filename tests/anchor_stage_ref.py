"""Plain CPU references for the steps between the tracker's first pass and its occlusion flags (csrc/anchors.hip and the
sampling / cosine part of csrc/core.hip), written from the layout comments of those files and of include/dtk.h: float64
wherever arithmetic is involved, float32 only where the device's COMPARISON is defined on the float32 value (cs >= th,
cs < cos_th, the TAP-Vid distance).  The input sets of tests/test_gpu_anchor_stage.py are generated here too, so that
tests/test_anchor_stage_reference.py can assert their conditions on the references alone.  Nothing here touches the library."""
from types import SimpleNamespace

import numpy as np
import torch

ANCHOR_TH, COS_TH = 0.7, 0.6
F32 = np.float32


# --------------------------------------------------------------------------------------------------------------
# dtk_build_anchor_sources
# --------------------------------------------------------------------------------------------------------------
def anchor_sources_ref(cs, th):
    """cs [N,T] float32, th -> n_anchors [N], pair_off [N+1], pair_frame [P], counts [3], src_row / tgt / out_idx [P*T].
    A_n = {a : cs[n][a] >= th} in float32 (NaN is never an anchor); pairs n-major, p = pair_off[n] + rank of a in A_n;
    sources sorted by anchor frame, within a frame by query; row j*T + t = (n*T + t, a, p*T + t)."""
    cs = np.asarray(cs, dtype=F32)
    N, T = cs.shape
    thf = F32(th)
    anchors = [[a for a in range(T) if cs[n, a] >= thf] for n in range(N)]
    n_anchors = np.array([len(a) for a in anchors], dtype=np.int32)
    pair_off = np.zeros(N + 1, dtype=np.int32)
    for n in range(N):
        pair_off[n + 1] = pair_off[n] + n_anchors[n]
    P = int(pair_off[N])
    pair_frame = np.zeros(P, dtype=np.int32)
    for n in range(N):
        for k, a in enumerate(anchors[n]):
            pair_frame[pair_off[n] + k] = a
    src_row, tgt, out_idx = (np.zeros(P * T, dtype=np.int32) for _ in range(3))
    j = 0
    for a in range(T):
        for n in range(N):
            if a in anchors[n]:
                p = pair_off[n] + anchors[n].index(a)
                for t in range(T):
                    src_row[j * T + t] = n * T + t
                    tgt[j * T + t] = a
                    out_idx[j * T + t] = p * T + t
                j += 1
    assert j == P
    counts = np.array([P, P * T, sum(1 for a in anchors if not a)], dtype=np.int32)
    return SimpleNamespace(n_anchors=n_anchors, pair_off=pair_off, pair_frame=pair_frame, counts=counts, src_row=src_row,
                           tgt=tgt, out_idx=out_idx)


# --------------------------------------------------------------------------------------------------------------
# dtk_occlusion
# --------------------------------------------------------------------------------------------------------------
def occlusion_ref(green, pair_off, pair_frame, traj, cs, anchor_th, cos_th):
    """green [P,T,2], pair_off [N+1], pair_frame [P], traj [N,T,2], cs [N,T] -> (occ [N,T] bool, margin [N,T] float64).
    d[k][t] = |green[p0+k][t] - traj[n][a_k]| in float64; med[t] = element (A-1)//2 of the sorted d[:, t]; tau = max of med
    over the frames with cs >= anchor_th; occ = med > tau or cs < cos_th (both cs comparisons on the float32 values).  A query
    without anchors is all ones (margin inf).  margin = |med - tau|."""
    green = np.asarray(green, dtype=np.float64)
    traj = np.asarray(traj, dtype=np.float64)
    cs = np.asarray(cs, dtype=F32)
    N, T = cs.shape
    occ = np.ones((N, T), dtype=bool)
    margin = np.full((N, T), np.inf)
    for n in range(N):
        p0, p1 = int(pair_off[n]), int(pair_off[n + 1])
        A = p1 - p0
        if A <= 0:
            continue
        frames = np.asarray(pair_frame[p0:p1], dtype=np.int64)
        diff = green[p0:p1] - traj[n][frames][:, None, :]  # [A,T,2]
        d = np.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1])
        med = np.sort(d, axis=0)[(A - 1) // 2]
        vis = cs[n] >= F32(anchor_th)
        tau = med[vis].max() if vis.any() else -np.inf
        occ[n] = (med > tau) | (cs[n] < F32(cos_th))
        margin[n] = np.abs(med - tau)
    return occ, margin


def anchor_counts_for(T):
    """anchors per query: 0, 1, 2, 3 (both parities, the one-element median), 64 / 65 / 129 (one, two and three lane strides of
    the 64-wide wave) and T, as far as they fit"""
    return sorted({c for c in (0, 1, 2, 3, 64, 65, 129, T) if c <= T})


def occlusion_cs(T, counts, rng):
    """cs [len(counts), T] float32 with exactly counts[n] entries >= 0.7f in row n, at random frames; where there is room one
    anchor sits exactly ON the anchor threshold and one other frame exactly ON the cosine threshold (visible)"""
    below = np.nextafter(F32(ANCHOR_TH), F32(0))
    cs = np.empty((len(counts), T), dtype=F32)
    for n, A in enumerate(counts):
        row = np.minimum(rng.uniform(0.3, 0.7, T).astype(F32), below)
        frames = rng.permutation(T)[:A]
        row[frames] = np.maximum(rng.uniform(0.7, 1.0, A).astype(F32), F32(ANCHOR_TH))
        if A >= 2:
            row[frames[0]] = F32(ANCHOR_TH)
        rest = np.setdiff1d(np.arange(T), frames)
        if rest.size:
            row[rest[0]] = F32(COS_TH)
        cs[n] = row
    return cs


def occlusion_case(T, kind, seed, counts=None):
    """One input set of the occlusion tests.  kind "int": integer pixel coordinates in [0, 64) -- squared distances are exact
    integers <= 8192 in either precision, so float32 and float64 order them identically and exact ties are plentiful; kind
    "cont": continuous uniform coordinates in a 854 x 476 frame.  pair_off / pair_frame come from anchor_sources_ref."""
    rng = np.random.default_rng(seed)
    counts = anchor_counts_for(T) if counts is None else list(counts)
    cs = occlusion_cs(T, counts, rng)
    src = anchor_sources_ref(cs, ANCHOR_TH)
    assert list(src.n_anchors) == list(counts)
    P, N = int(src.counts[0]), len(counts)
    if kind == "int":
        green = rng.integers(0, 64, (P, T, 2)).astype(F32)
        traj = rng.integers(0, 64, (N, T, 2)).astype(F32)
    else:
        size = np.array([854.0, 476.0])
        green = (rng.random((P, T, 2)) * size).astype(F32)
        traj = (rng.random((N, T, 2)) * size).astype(F32)
    return SimpleNamespace(T=T, N=N, kind=kind, cs=cs, pair_off=src.pair_off, pair_frame=src.pair_frame, green=green, traj=traj,
                           counts=counts)


# name -> (T, kind, seed, counts); counts None = anchor_counts_for(T).  The seeds of the "cont" sets are vetted by
# tests/test_anchor_stage_reference.py::test_input_set_conditions.
def _many_counts():
    c = np.random.default_rng(7).integers(0, 9, 300)
    c[:9] = np.arange(9)
    return c


OCCLUSION_CASES = {}
for _T in (1, 2, 5, 63, 64, 65, 130, 257, 300):
    for _kind in ("int", "cont"):
        OCCLUSION_CASES[f"T{_T}_{_kind}"] = (_T, _kind, 1000 + _T, None)
for _kind in ("int", "cont"):
    OCCLUSION_CASES[f"N300_T8_{_kind}"] = (8, _kind, 2008, _many_counts())
    OCCLUSION_CASES[f"T3072_{_kind}"] = (3072, _kind, 4072, [3])  # the largest T dtk_occlusion accepts (60 KB of LDS)

_occ_cache = {}


def occlusion_inputs(name):
    """(case, occ, margin) of OCCLUSION_CASES[name]; computed once and shared, never modified"""
    if name not in _occ_cache:
        T, kind, seed, counts = OCCLUSION_CASES[name]
        case = occlusion_case(T, kind, seed, counts)
        occ, margin = occlusion_ref(case.green, case.pair_off, case.pair_frame, case.traj, case.cs, ANCHOR_TH, COS_TH)
        _occ_cache[name] = (case, occ, margin)
    return _occ_cache[name]


# --------------------------------------------------------------------------------------------------------------
# dtk_traj_cos_sims, dtk_sample_points, dtk_sample_grid
# --------------------------------------------------------------------------------------------------------------
def cos_sims_ref(S, tq, eps=1e-8):
    """S [N,T,C], tq [N] (clamped into [0, T-1]) -> cs [N,T] float64 = <a,b> / (max(|a|, eps) max(|b|, eps)), a = S[n][tq[n]]"""
    S = np.asarray(S, dtype=np.float64)
    N, T, _ = S.shape
    q = np.clip(np.asarray(tq, dtype=np.int64), 0, T - 1)
    a = S[np.arange(N), q][:, None, :]
    ab = (a * S).sum(-1)
    na = np.maximum(np.sqrt((a * a).sum(-1)), eps)
    nb = np.maximum(np.sqrt((S * S).sum(-1)), eps)
    return ab / (na * nb)


def sample_points_ref(feat, ph, pw, patch, stride, xy, t_idx):
    """feat [T, ph*pw, C] token-major, xy [B,2] pixels, t_idx [B] -> [B,C] float64.  u = (x - patch/2) / stride clamped to
    [0, pw-1] (border), u0 = floor(u), u1 = min(u0 + 1, pw-1); the same in y; t clamped into [0, T-1]."""
    feat = np.asarray(feat, dtype=np.float64)
    T = feat.shape[0]
    vol = feat.reshape(T, ph, pw, -1)
    xy = np.asarray(xy, dtype=np.float64)
    u = np.clip((xy[:, 0] - patch / 2) / stride, 0, pw - 1)
    v = np.clip((xy[:, 1] - patch / 2) / stride, 0, ph - 1)
    u0, v0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fu, fv = (u - u0)[:, None], (v - v0)[:, None]
    u1, v1 = np.minimum(u0 + 1, pw - 1), np.minimum(v0 + 1, ph - 1)
    t = np.clip(np.asarray(t_idx, dtype=np.int64), 0, T - 1)
    top = vol[t, v0, u0] * (1 - fu) + vol[t, v0, u1] * fu
    bot = vol[t, v1, u0] * (1 - fu) + vol[t, v1, u1] * fu
    return top * (1 - fv) + bot * fv


def sample_grid_ref(feat, ph, pw, pts):
    """feat [T, ph*pw, C] token-major, pts [B,3] = (x, y, t) in grid_sample coordinates -> [B,C] float64: F.grid_sample of the
    1 x C x T x ph x pw volume, trilinear, align_corners=True, padding_mode='border'"""
    import torch.nn.functional as F
    feat = torch.as_tensor(np.asarray(feat)).double()
    T, _, C = feat.shape
    vol = feat.reshape(T, ph, pw, C).permute(3, 0, 1, 2)[None]
    grid = torch.as_tensor(np.asarray(pts)).double()[None, None, :, None, :]
    out = F.grid_sample(vol, grid, mode="bilinear", align_corners=True, padding_mode="border")  # [1,C,1,B,1]
    return out[0, :, 0, :, 0].T.contiguous().numpy()


# --------------------------------------------------------------------------------------------------------------
# dtk_tapvid_counts
# --------------------------------------------------------------------------------------------------------------
def tapvid_counts_ref(pred, pred_occ, gt, gt_occ, qframe, pred_size, gt_size, query_mode="strided"):
    """The 18 counts of one video: [0] evaluated points, [1] occlusion prediction == ground truth, [2] visible in the ground
    truth, then per threshold 2^i px: within & visible, within & visible & predicted visible, false positives -- over the
    evaluated frames (strided: t != query frame; first: t > query frame).  Both track sets are scaled to 256 x 256 and the
    squared distance is summed in float32, compared strictly with the squared threshold."""
    pred = np.array(pred, dtype=F32)
    gt = np.array(gt, dtype=F32)
    N, T = pred.shape[:2]
    sp = [F32(256 / pred_size[0]), F32(256 / pred_size[1])]
    sg = [F32(256 / gt_size[0]), F32(256 / gt_size[1])]
    dx = pred[..., 0] * sp[0] - gt[..., 0] * sg[0]
    dy = pred[..., 1] * sp[1] - gt[..., 1] * sg[1]
    d2 = dx * dx + dy * dy
    assert d2.dtype == F32
    vis = ~np.asarray(gt_occ).astype(bool).reshape(N, T)
    pvis = ~np.asarray(pred_occ).astype(bool).reshape(N, T)
    ts = np.arange(T)[None, :]
    qf = np.asarray(qframe, dtype=np.int64).reshape(N, 1)
    ev = (ts > qf) if query_mode == "first" else (ts != qf)
    counts = [int(ev.sum()), int(((pvis == vis) & ev).sum()), int((vis & ev).sum())]
    for th in (1, 2, 4, 8, 16):
        within = d2 < F32(th * th)
        counts += [int((within & vis & ev).sum()), int((within & vis & pvis & ev).sum()),
                   int(((((~vis) & pvis) | ((~within) & pvis)) & ev).sum())]
    return counts


def metrics_from_counts_ref(counts):
    """the ratios eval/metrics.py forms from the sums above"""
    ev, occ_eq, vis = counts[:3]
    out = {"occlusion_accuracy": occ_eq / ev}
    jac, frac = [], []
    for i, th in enumerate((1, 2, 4, 8, 16)):
        correct, tp, fp = counts[3 + 3 * i:6 + 3 * i]
        out[f"pts_within_{th}"] = correct / vis
        out[f"jaccard_{th}"] = tp / (vis + fp)
        frac.append(out[f"pts_within_{th}"])
        jac.append(out[f"jaccard_{th}"])
    out["average_jaccard"] = float(np.mean(jac))
    out["average_pts_within_thresh"] = float(np.mean(frac))
    return out
