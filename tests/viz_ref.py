"""The picture of docs/RENDER.md restated in numpy: primitive generation for the dotted and the trail videos, and a brute-force
blend that visits every primitive at every pixel in draw order.  float64 by default; `dtype=np.float32` runs the SAME code in
float32 (every constant and every intermediate), which is how the device bounds of docs/PARITY.md are derived
(tests/test_viz_reference.py::test_float32_against_float64 prints them).

A record is a row of 12 numbers (include/dtk.h): kind, x0, y0, x1, y1, size, r, g, b, a, 1 / |p1 - p0|^2, frame.  Here kind and
frame are plain numbers; `device_records` packs them into the int32 bit patterns the library reads.
"""
import colorsys

import numpy as np

SEGMENT, DISC, DIAMOND = 0, 1, 2
K_PT = 64.0 / 72.0            # pixels per point at the reference's figure_dpi = 64
KIND = {"o": DISC, "D": DIAMOND}


def half_width(linewidth):
    return linewidth * K_PT / 2.0


def marker_size(marker, s):
    """radius of the disc 'o' / L1 radius rho of the diamond 'D' for scatter size s (points^2)."""
    if marker == "o":
        return np.sqrt(s) * K_PT / 2.0
    if marker == "D":
        return np.sqrt(s) * K_PT * np.sqrt(2.0) / 2.0
    raise NotImplementedError(marker)


def rainbow(N):
    return np.array([colorsys.hsv_to_rgb(n / N, 1.0, 1.0) for n in range(N)], dtype=np.float64).reshape(N, 3)


def frame_maps(homogs):
    """[T, T, 3, 3] float64: maps[i, j] = inv(H_i) H_j, as reference :730 forms it."""
    homogs = np.asarray(homogs, dtype=np.float64)
    inv = np.stack([np.linalg.inv(h) for h in homogs])
    return np.stack([np.stack([np.matmul(inv[i], homogs[j]) for j in range(len(homogs))]) for i in range(len(homogs))])


def clamp_points(points, H, W, dt):
    p = np.asarray(points).astype(dt)
    p = np.maximum(p, dt(0))
    return np.minimum(p, np.array([W, H], dtype=dt))


def _records(kind, p0, p1, size, colors, a, frame, dt):
    n = len(a)
    d = p1 - p0
    len2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(len2 > 0, dt(1) / len2, dt(0)).astype(dt)
    rec = np.zeros((n, 12), dtype=dt)
    rec[:, 0] = kind
    rec[:, 1:3], rec[:, 3:5] = p0, p1
    rec[:, 5] = dt(size)
    rec[:, 6:9] = colors.astype(dt)
    rec[:, 9] = a
    rec[:, 10] = inv if kind == SEGMENT else 0
    rec[:, 11] = frame
    return rec


def dotted_prims(points, occluded, H, W, i, point_size, marker="o", colors=None, frame=0, dtype=np.float64):
    """plot_tracks_v2, frame i: one marker per point in ascending n, a = 1 - occluded[n, i]."""
    dt = dtype
    N = points.shape[0]
    colors = rainbow(N) if colors is None else np.asarray(colors, dtype=np.float64)
    p = clamp_points(points, H, W, dt)[:, i]
    a = (dt(1) - (np.asarray(occluded)[:, i] != 0).astype(dt))
    return _records(KIND[marker], p, p, marker_size(marker, point_size), colors, a, frame, dt)


def tail_prims(points, occluded, maps, H, W, i, point_size, linewidth, marker="o", colors=None, trail_fade=True, frame=0,
               dtype=np.float64):
    """plot_tracks_tails :716-767, frame i: the markers, then for j = i - 1 .. 0 the N segments P(n, j) -> P(n, j + 1)."""
    dt = dtype
    N = points.shape[0]
    colors = rainbow(N) if colors is None else np.asarray(colors, dtype=np.float64)
    pts = clamp_points(points, H, W, dt)
    occ = (np.asarray(occluded) != 0).astype(dt)
    lim = np.array([W, H], dtype=dt)
    out = [_records(KIND[marker], pts[:, i], pts[:, i], marker_size(marker, point_size), colors, dt(1) - occ[:, i], frame, dt)]

    def mapped(j):
        if j == i:
            return pts[:, i]
        m = np.asarray(maps[i, j]).astype(dt).reshape(9)
        x, y = pts[:, j, 0], pts[:, j, 1]
        X = m[0] * x + m[1] * y + m[2]
        Y = m[3] * x + m[4] * y + m[5]
        w = m[6] * x + m[7] * y + m[8]
        den = np.maximum(dt(1e-12), np.abs(w)) * np.sign(w)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.stack([X / den, Y / den], axis=1)

    for j in range(i - 1, -1, -1):
        p0, p1 = mapped(j), mapped(j + 1)
        both = np.stack([p0, p1], axis=1)
        oof = np.logical_or(both < dt(1), both > lim).any(axis=(1, 2))
        p0c = np.minimum(np.maximum(p0, dt(1)), lim - dt(1))
        p1c = np.minimum(np.maximum(p1, dt(1)), lim - dt(1))
        a = (dt(1) - occ[:, j]) * (dt(1) - occ[:, j + 1]) * (dt(1) - oof.astype(dt))
        if trail_fade:
            a = a * max(dt(1) - dt(0.9) * (dt(i - j) / (dt(i + 1) * dt(0.99))), dt(0.1))
        out.append(_records(SEGMENT, p0c, p1c, half_width(linewidth), colors, a.astype(dt), frame, dt))
    return np.concatenate(out)


def drawn(rec):
    """the records that draw: a > 0 and every coordinate finite (docs/RENDER.md: the others are skipped)."""
    return (rec[:, 9] > 0) & np.isfinite(rec[:, 1:6]).all(axis=1)


def coverage(r, X, Y, dt):
    ax, ay = X - r[1], Y - r[2]
    if int(r[0]) == DIAMOND:
        cov = dt(0.5) + (r[5] - np.abs(ax) - np.abs(ay)) / dt(np.sqrt(2.0))
    else:
        dx, dy = r[3] - r[1], r[4] - r[2]
        t = np.clip((ax * dx + ay * dy) * r[10], dt(0), dt(1))
        ex, ey = ax - t * dx, ay - t * dy
        cov = dt(0.5) + r[5] - np.sqrt(ex * ex + ey * ey)
    return np.clip(cov, dt(0), dt(1)).astype(dt)


def blend(frame_u8, rec, dtype=np.float64):
    """[H, W, 3] in [0, 1]: frame / 255 blended with EVERY record of `rec` (already of `dtype`) in order, at every pixel."""
    dt = dtype
    H, W = frame_u8.shape[:2]
    c = frame_u8.astype(dt) / dt(255)
    Y, X = np.meshgrid(np.arange(H, dtype=dt), np.arange(W, dtype=dt), indexing="ij")
    rec = np.asarray(rec).astype(dt)
    keep = drawn(rec)
    for r in rec[keep]:
        w = (r[9] * coverage(r, X, Y, dt))[..., None]
        c = c * (dt(1) - w) + r[6:9] * w
    return c.astype(dt)


def to_u8(c):
    return np.floor(255.0 * c + 0.5).astype(np.uint8)


def device_records(rec):
    """float32 [P, 12] with kind and frame as int32 bit patterns: what ops.render_* take."""
    rec = np.asarray(rec)
    out = np.ascontiguousarray(rec.astype(np.float32))
    bits = out.view(np.int32)
    bits[:, 0] = rec[:, 0].astype(np.int32)
    bits[:, 11] = rec[:, 11].astype(np.int32)
    return out


def video(rgb, points, occluded, homogs, point_size, linewidth=1.5, marker="o", colors=None, trail_fade=True, tails=True,
          dtype=np.float64):
    """The whole video in [0, 1]: [T, H, W, 3] of `dtype`."""
    T, H, W = rgb.shape[:3]
    maps = frame_maps(homogs) if tails else None
    out = []
    for i in range(T):
        rec = (tail_prims(points, occluded, maps, H, W, i, point_size, linewidth, marker, colors, trail_fade, dtype=dtype) if tails
               else dotted_prims(points, occluded, H, W, i, point_size, marker, colors, dtype=dtype))
        out.append(blend(rgb[i], rec, dtype))
    return np.stack(out)


# ---- scenes shared by tests/test_viz_reference.py (float32-against-float64 figures) and tests/test_gpu_render.py -------------------
def exact_mask(frame_shape, rec):
    """[H, W] bool: pixels whose float64 result is a pure selection -- after the last primitive that covers the pixel EXACTLY
    (coverage 1, opaque), every later one has coverage exactly 0 or 1.  There the blend is c <- colour or c <- c, exact in any
    precision and any operation order; `rec` must be opaque (a = 1 or 0)."""
    H, W = frame_shape
    Y, X = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rec = np.asarray(rec, dtype=np.float64)
    exact = np.ones((H, W), dtype=bool)
    for r in rec[drawn(rec)]:
        assert r[9] == 1.0
        cov = coverage(r, X, Y, np.float64)
        exact = np.where(cov == 1.0, True, exact & ~((cov > 0) & (cov < 1)))
    return exact


def _rec(kind, x0, y0, x1, y1, size, rgb, a=1.0, frame=0):
    d2 = (x1 - x0) ** 2 + (y1 - y0) ** 2
    return [kind, x0, y0, x1, y1, size, rgb[0], rgb[1], rgb[2], a, (1.0 / d2 if d2 > 0 and kind == SEGMENT else 0.0), frame]


def exact_scene(H=50, W=70):
    """Opaque primitives on integer coordinates, 70 x 50 (ragged tiles on both edges), two frames; float32-representable.
    Frame 0: 600 overlapping primitives inside tile (1, 1) (more than two LDS chunks of 256), a fat diagonal across the whole
    frame, primitives wholly outside the frame, a zero-length segment.  Frame 1: no primitive at all."""
    rng = np.random.default_rng(5)
    pal = np.round(rng.random((64, 3)) * 255) / 255
    rows = [_rec(SEGMENT, 0, 0, W - 1, H - 1, 2.5, pal[0])]
    for k in range(600):
        kind = (SEGMENT, SEGMENT, SEGMENT, DISC, SEGMENT, SEGMENT, SEGMENT, DIAMOND)[k % 8]
        x0, y0 = rng.integers(18, 30, size=2)
        if kind == SEGMENT:
            length = int(rng.integers(0, 6))
            x1, y1 = (min(x0 + length, 29), y0) if k % 16 < 8 else (x0, min(y0 + length, 29))
            rows.append(_rec(kind, x0, y0, x1, y1, 0.5 + int(rng.integers(0, 2)), pal[1 + k % 63]))
        else:
            rows.append(_rec(kind, x0, y0, x0, y0, 0.5 + int(rng.integers(1, 3)), pal[1 + k % 63]))
    rows.append(_rec(SEGMENT, -20, -5, -10, -5, 2.5, pal[3]))      # wholly outside
    rows.append(_rec(DISC, W + 30, 25, W + 30, 25, 6.5, pal[4]))
    rows.append(_rec(DIAMOND, 35, H + 40, 35, H + 40, 8.5, pal[5]))
    rows.append(_rec(SEGMENT, 50, 40, 50, 40, 3.5, pal[6]))        # zero length: a disc
    rows.append(_rec(SEGMENT, 60, 5, 69, 5, 1.5, pal[7]))          # touches the ragged right edge
    rows.append(_rec(DIAMOND, 8, 45, 8, 45, 6.5, pal[8]))          # crosses the ragged bottom edge
    rec = np.array(rows, dtype=np.float64).astype(np.float32)
    frames = rng.integers(0, 256, size=(2, H, W, 3)).astype(np.uint8)
    return frames, rec


def numeric_scene(H=50, W=80, n=300, seed=9):
    """300 random primitives of the three kinds with a in (0, 1) on 80 x 50, some partly or wholly outside; float32 values."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        kind = k % 3
        x0, y0 = rng.uniform(-6, W + 6), rng.uniform(-6, H + 6)
        a, rgb = rng.uniform(0.05, 0.95), rng.random(3)
        if kind == SEGMENT:
            ang, length = rng.uniform(0, 2 * np.pi), rng.uniform(0, 25)
            x1, y1 = x0 + length * np.cos(ang), y0 + length * np.sin(ang)
            x0, y0, x1, y1 = (np.float32(v) for v in (x0, y0, x1, y1))
            rows.append(_rec(kind, float(x0), float(y0), float(x1), float(y1), rng.uniform(0.3, 2.5), rgb, a))
        else:
            x0, y0 = float(np.float32(x0)), float(np.float32(y0))
            rows.append(_rec(kind, x0, y0, x0, y0, rng.uniform(0.5, 6.0), rgb, a))
    rec = np.array(rows, dtype=np.float64).astype(np.float32)
    d = rec[:, 3:5].astype(np.float64) - rec[:, 1:3].astype(np.float64)
    len2 = (d * d).sum(axis=1)
    rec[:, 10] = np.where((rec[:, 0] == SEGMENT) & (len2 > 0), 1.0 / np.maximum(len2, 1e-300), 0.0).astype(np.float32)
    frame = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    return frame, rec
