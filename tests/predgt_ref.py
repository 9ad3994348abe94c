"""The prediction-against-ground-truth picture of docs/RENDER.md section 5 and the BADJA counts restated in numpy, on top of
tests/viz_ref.py: the two records per (frame, point) of the four occlusion cases, the ring coverage, a brute-force blend and the
exact-selection mask that know the ring, the translation of records back into the reference's cv2 calls (tests/golden/predgt.npz),
the frame filter, and compute_badja_metrics_for_video as three integer counts.  float64 by default; `dtype=np.float32` runs the
same code in float32, which is how the device bounds of docs/PARITY.md are derived."""
import numpy as np

import viz_ref as R

SEGMENT, DISC, DIAMOND, RING = 0, 1, 2, 3
RED = (1.0, 0.0, 0.0)


# ---- records ---------------------------------------------------------------------------------------------------------------------
def int_points(x):
    """tuple(point.astype(int)): truncation toward zero."""
    return np.asarray(x).astype(int)


def _row(kind, x0, y0, x1, y1, size, rgb, a, w10, frame, dt):
    return np.array([kind, x0, y0, x1, y1, size, rgb[0], rgb[1], rgb[2], a, w10, frame], dtype=dt)


def _segment(p0, p1, hw, rgb, frame, dt):
    d = np.array([p1[0] - p0[0], p1[1] - p0[1]], dtype=dt)
    len2 = d[0] * d[0] + d[1] * d[1]
    return _row(SEGMENT, p0[0], p0[1], p1[0], p1[1], hw, rgb, 1, (dt(1) / len2) if len2 > 0 else 0, frame, dt)


def pred_gt_records(pred_xy, gt_xy, pred_occ, gt_occ, colors, i, thickness=4, radius=8, cross_size=8, frame=0, dtype=np.float64):
    """overlay_pred_gt_on_frame (visualize_pred_vs_gt.py:21-38) for frame i: [2 N, 12], two records per point in ascending n.
    pred_xy / gt_xy [N, T, 2] integers, colors [N, 3] in [0, 1]."""
    dt = dtype
    out = []
    for n in range(len(pred_xy)):
        p, g = pred_xy[n, i].astype(dt), gt_xy[n, i].astype(dt)
        col = np.asarray(colors[n], dtype=np.float64).astype(dt)
        pocc, gocc = bool(pred_occ[n, i]), bool(gt_occ[n, i])
        if pocc and gocc:
            out += [_row(SEGMENT, 0, 0, 0, 0, 0, (0, 0, 0), 0, 0, frame, dt)] * 2
        elif gocc:
            r = dt(cross_size)
            out.append(_segment((p[0] - r, p[1] - r), (p[0] + r, p[1] + r), dt(thickness) / 2, col, frame, dt))
            out.append(_segment((p[0] - r, p[1] + r), (p[0] + r, p[1] - r), dt(thickness) / 2, col, frame, dt))
        elif pocc:
            out.append(_segment(p, g, dt(thickness // 2) / 2, RED, frame, dt))
            out.append(_row(RING, p[0], p[1], p[0], p[1], radius, col, 1, 1, frame, dt))       # cv2 thickness 2: hw = 1
        else:
            out.append(_segment(p, g, dt(thickness) / 2, RED, frame, dt))
            out.append(_row(DISC, p[0], p[1], p[0], p[1], radius, col, 1, 0, frame, dt))
    return np.stack(out).astype(dt)


def calls_of(rec, pos, source_frame):
    """The records of one frame as rows of the golden's call arrays: position, kind (0 line, 1 circle), x0, y0, x1, y1, radius,
    cv2 thickness, r, g, b (0 .. 255), source frame.  Records with a = 0 are no call."""
    rows = []
    for r in rec:
        if r[9] == 0:
            continue
        rgb = [int(round(float(v) * 255)) for v in r[6:9]]
        kind = int(r[0])
        if kind == SEGMENT:
            rows.append([pos, 0, int(r[1]), int(r[2]), int(r[3]), int(r[4]), 0, int(round(2 * float(r[5])))] + rgb + [source_frame])
        else:
            assert kind in (DISC, RING)
            th = -1 if kind == DISC else int(round(2 * float(r[10])))
            rows.append([pos, 1, int(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[5]), th] + rgb + [source_frame])
    return np.array(rows, dtype=np.int64).reshape(-1, 12)


def badja_frames(gt):
    """visualize_pred_vs_gt.py:51."""
    gt = np.asarray(gt)
    return [i for i in range(gt.shape[1]) if ((gt[:, i, :] < 1).all(axis=-1)).mean() < 0.6]


# ---- coverage, blend, exact mask: viz_ref's, plus the ring -----------------------------------------------------------------------------
def coverage(r, X, Y, dt):
    if int(r[0]) != RING:
        return R.coverage(r, X, Y, dt)
    ax, ay = X - r[1], Y - r[2]
    cov = dt(0.5) + r[10] - np.abs(np.sqrt(ax * ax + ay * ay) - r[5])
    return np.clip(cov, dt(0), dt(1)).astype(dt)


def drawn(rec):
    return R.drawn(rec) & np.isfinite(rec[:, 10])


def blend(frame_u8, rec, dtype=np.float64):
    """viz_ref.blend with the ring: frame / 255 blended with every record in order, at every pixel."""
    dt = dtype
    H, W = frame_u8.shape[:2]
    c = frame_u8.astype(dt) / dt(255)
    Y, X = np.meshgrid(np.arange(H, dtype=dt), np.arange(W, dtype=dt), indexing="ij")
    rec = np.asarray(rec).astype(dt)
    for r in rec[drawn(rec)]:
        w = (r[9] * coverage(r, X, Y, dt))[..., None]
        c = c * (dt(1) - w) + r[6:9] * w
    return c.astype(dt)


def exact_mask(frame_shape, rec):
    """viz_ref.exact_mask with the ring: pixels where the float64 result is a pure selection."""
    H, W = frame_shape
    Y, X = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rec = np.asarray(rec, dtype=np.float64)
    exact = np.ones((H, W), dtype=bool)
    for r in rec[drawn(rec)]:
        assert r[9] == 1.0
        cov = coverage(r, X, Y, np.float64)
        exact = np.where(cov == 1.0, True, exact & ~((cov > 0) & (cov < 1)))
    return exact


def grow(rec):
    """how far the bounding box of each record is grown before binning (docs/RENDER.md), as the device's float32 constants."""
    rec = np.asarray(rec, dtype=np.float64)
    g = rec[:, 5] + np.where(rec[:, 0] == DIAMOND, np.float64(np.float32(0.70711)), 0.5)
    return g + np.where(rec[:, 0] == RING, rec[:, 10], 0.0)


def tile_counts(rec, H, W, tile=16):
    """number of tiles the grown box, clipped to the frame, meets; 0 for a box outside the frame or a <= 0."""
    rec = np.asarray(rec, dtype=np.float64)
    g = grow(rec)
    lo = np.minimum(rec[:, 1:3], rec[:, 3:5]) - g[:, None]
    hi = np.maximum(rec[:, 1:3], rec[:, 3:5]) + g[:, None]
    lim = np.array([W - 1, H - 1], dtype=np.float64)
    visible = (hi >= 0).all(axis=1) & (lo <= lim).all(axis=1) & (rec[:, 9] > 0)
    t0 = np.floor(np.maximum(lo, 0)).astype(np.int64) // tile
    t1 = np.ceil(np.minimum(hi, lim)).astype(np.int64) // tile
    return np.where(visible, (t1 - t0 + 1).prod(axis=1), 0)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def ring_row(x, y, r, hw, rgb, a=1.0, frame=0):
    return [RING, x, y, x, y, r, rgb[0], rgb[1], rgb[2], a, hw, frame]


def exact_scene():
    """viz_ref.exact_scene (70 x 50, two frames, 600 opaque primitives on integer coordinates inside tile (1, 1)) with every disc
    among the first 400 crowded primitives turned into a ring, plus a ring of radius 8 around (52, 20), one across the left edge
    and one wholly outside.  The later primitives of the crowded tile paint over most of the rings' one-pixel ramps, so the tile
    keeps pixels that are pure selections."""
    frames, rec = R.exact_scene()
    rec = rec.astype(np.float64)
    rings = 0
    for k in range(1, 401):
        if rec[k, 0] == DISC:
            rec[k, 0], rec[k, 5], rec[k, 10] = RING, 1 + rings % 3, (0.5, 1.0)[rings % 2]
            rings += 1
    pal = np.array([[51, 204, 102], [230, 153, 26], [128, 128, 128]]) / 255   # n / 255, like viz_ref's palette: away from the
    extra = [ring_row(52, 20, 8, 1.0, pal[0]), ring_row(-2, 30, 6, 1.0, pal[1]),  # rounding boundaries of the uint8 output
             ring_row(-30, -30, 8, 1.0, pal[2])]
    rec = np.concatenate([rec, np.array(extra, dtype=np.float64)])
    assert rings >= 40
    return frames, rec.astype(np.float32)


def numeric_scene(H=50, W=80, n=300, seed=19):
    """300 random primitives of the FOUR kinds with a in (0, 1) on 80 x 50, some partly or wholly outside; float32 values."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        kind = k % 4
        x0, y0 = float(np.float32(rng.uniform(-6, W + 6))), float(np.float32(rng.uniform(-6, H + 6)))
        a, rgb = rng.uniform(0.05, 0.95), rng.random(3)
        if kind == SEGMENT:
            ang, length = rng.uniform(0, 2 * np.pi), rng.uniform(0, 25)
            x1, y1 = float(np.float32(x0 + length * np.cos(ang))), float(np.float32(y0 + length * np.sin(ang)))
            rows.append(R._rec(kind, x0, y0, x1, y1, rng.uniform(0.3, 2.5), rgb, a))
        elif kind == RING:
            rows.append(ring_row(x0, y0, rng.uniform(1.0, 9.0), rng.uniform(0.3, 2.0), rgb, a))
        else:
            rows.append(R._rec(kind, x0, y0, x0, y0, rng.uniform(0.5, 6.0), rgb, a))
    rec = np.array(rows, dtype=np.float64).astype(np.float32)
    d = rec[:, 3:5].astype(np.float64) - rec[:, 1:3].astype(np.float64)
    len2 = (d * d).sum(axis=1)
    seg = rec[:, 0] == SEGMENT
    rec[seg, 10] = np.where(len2[seg] > 0, 1.0 / np.maximum(len2[seg], 1e-300), 0.0).astype(np.float32)
    frame = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    return frame, rec


def golden_records(gold, colors01, kept, dtype=np.float64):
    """the records of the golden scene, one array per kept frame."""
    pxy, gxy = int_points(gold["scene_pred"]), int_points(gold["scene_gt"])
    return [pred_gt_records(pxy, gxy, gold["scene_pred_occ"], gold["scene_gt_occ"], colors01, int(i), int(gold["thickness"]),
                            int(gold["radius"]), int(gold["cross_size"]), dtype=dtype) for i in kept]


# ---- BADJA -----------------------------------------------------------------------------------------------------------------------
def badja_counts(pred, gt, gt_occluded, seg, scale=(1.0, 1.0)):
    """eval/metrics.py:266-283 as (visible, dist < thr[t], dist < 3.0): float32 predictions scaled in float32, float64 ground
    truth, the float32 threshold float32(0.2) sqrt(float32(area[t]))."""
    pred = np.array(pred, dtype=np.float32)
    pred[..., 0] *= np.float32(scale[0])
    pred[..., 1] *= np.float32(scale[1])
    gt = np.asarray(gt, dtype=np.float64)
    seg = np.asarray(seg)
    t_seg = seg.shape[0]
    area = (seg > 0).reshape(t_seg, -1).sum(axis=1)
    thr = (np.float32(0.2) * np.sqrt(area.astype(np.float32))).astype(np.float32)
    d = pred.astype(np.float64) - gt
    dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])[:, 1:t_seg]
    vis = (np.asarray(gt_occluded)[:, 1:t_seg] == 0)
    return (int(vis.sum()), int((vis & (dist < thr[None, 1:].astype(np.float64))).sum()), int((vis & (dist < 3.0)).sum()))


def badja_metrics(counts):
    v, s, p = counts
    return {"acc_seg": 100.0 * s / v if v else float("nan"), "acc_3px": 100.0 * p / v if v else float("nan")}


def golden_badja(gold, which):
    """(pred, gt, occ) concatenated over the golden's start frames in its dict order; which = 'none' or '854'."""
    frames = [int(f) for f in gold["badja_frames"]]
    return (np.concatenate([gold[f"badja_pred_{which}_{f}"] for f in frames]), np.concatenate([gold[f"badja_gt_{f}"] for f in frames]),
            np.concatenate([gold[f"badja_occ_{f}"] for f in frames]))


def random_badja(n=2000, t=7, t_seg=6, h=40, w=56, seed=3, rel=1e-6):
    """2 000 points whose float64 distances stay `rel` (relative) away from 3.0 and from their frame's threshold; the entries that
    come too close are marked occluded, which takes them out of every count."""
    rng = np.random.default_rng(seed)
    seg = (rng.random((t_seg, h, w)) < rng.uniform(0.05, 0.6, size=(t_seg, 1, 1))).astype(np.uint8) * 255
    gt = rng.uniform(0, [w, h], size=(n, t, 2))
    pred = (gt + rng.normal(0, 2.5, size=gt.shape)).astype(np.float32)
    occ = rng.random((n, t)) < 0.3
    thr = np.float32(0.2) * np.sqrt((seg > 0).reshape(t_seg, -1).sum(1).astype(np.float32))
    d = pred.astype(np.float64) - gt
    dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    for t_i in range(1, t_seg):
        for edge in (3.0, float(thr[t_i])):
            occ[:, t_i] |= np.abs(dist[:, t_i] - edge) <= rel * edge
    return pred, gt, occ, seg
