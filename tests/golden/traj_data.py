"""Seeded inputs of the flow-trajectory fixtures (tests/golden/traj.npz, written by make_golden_traj.py).

Everything here is integer arithmetic or IEEE +, -, *, / on numpy float64 arrays followed by one rounding to float32 (no
transcendental functions; the random numbers are Generator.integers / Generator.random), so the arrays are bit-identical on every
machine; traj.npz pins their sha256 digests and the tests check them before comparing outputs.

Every case is a dict: fflow / bflow [T - 1, 2, h, w] float32 (frame i -> i + 1 and i + 1 -> i), direct = a list with, per starting
frame s < T - 1, the (forward, backward) flows [T - 1 - s, 2, h, w] from s to every later frame and back.

* `lattice()` -- T = 6, 17 x 33: h - 1 and w - 1 are powers of two and every flow is a multiple of 1/2, so every quantity of the
  chaining is a short dyadic number and exact in fp32, whatever the order of operations.  A rectangle moves by (-2, +1) per frame
  over a background moving by (+1, 0); ~6 % of the pixels carry integer noise in [-2, 2] and ~3 % half-integer noise (torch.round
  is half to even: 2.5 -> 2).  Content disoccludes and leaves the image, and cycle errors of exactly 1.0 occur (strict <).
* `smooth(seed, T, h, w)` -- an affine motion per frame plus 0.15 px noise, plus a disc of 12 x the noise where the flows
  disagree; the direct flows are the composed affine maps plus noise plus a drift that grows with the frame distance on one
  side of the image, so that the direct filter bites.  SMOOTH is the committed small case, MID the one that crosses block borders.
"""
import hashlib

import numpy as np

THRESHOLD, DIRECT_THRESHOLD = 1.0, 1.5
LATTICE = dict(T=6, h=17, w=33)
SMOOTH = dict(seed=20261017, T=7, h=23, w=41)
MID = dict(seed=12200, T=12, h=120, w=200)


def digest(a: np.ndarray) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def case_digest(case) -> str:
    parts = [case["fflow"], case["bflow"]] + [x for pair in case["direct"] for x in pair]
    return digest(np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in parts]))


def _grid(h, w):
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return xx, yy


# ---- lattice --------------------------------------------------------------------------------------------------------------------
def _rect(t, h, w):
    """the rectangle at frame t: x in [20 - 2 t, 28 - 2 t), y in [3 + t, 9 + t)"""
    xx, yy = _grid(h, w)
    return (xx >= 20 - 2 * t) & (xx < 28 - 2 * t) & (yy >= 3 + t) & (yy < 9 + t)


def _lattice_noise(rng, shape):
    """integer noise in [-2, 2] on ~6 % of the pixels, odd multiples of 1/2 in [-1.5, 1.5] on ~3 %"""
    u = rng.random(shape[-2:])
    whole = rng.integers(-2, 3, size=shape).astype(np.float64)
    half = rng.integers(-2, 2, size=shape).astype(np.float64) + 0.5
    out = np.zeros(shape)
    out = np.where(u < 0.06, whole, out)
    return np.where((u >= 0.06) & (u < 0.09), half, out)


def lattice():
    T, h, w = LATTICE["T"], LATTICE["h"], LATTICE["w"]
    rng = np.random.default_rng(1733)

    _, yy = _grid(h, w)

    def field(mask, fg, bg, steps=1, drift_rows=0, drift=0.0):
        f = np.empty((2, h, w))
        f[0] = np.where(mask, fg[0] * steps, bg[0] * steps)
        f[1] = np.where(mask, fg[1] * steps, bg[1] * steps)
        if steps >= 3:   # the direct flows over three frames or more disagree with the chain by 2 px in the upper rows
            f[1] += np.where(yy < drift_rows, drift, 0.0)
        return f + _lattice_noise(rng, (2, h, w))

    fflow = np.stack([field(_rect(i, h, w), (-2, 1), (1, 0)) for i in range(T - 1)])
    bflow = np.stack([field(_rect(i + 1, h, w), (2, -1), (-1, 0)) for i in range(T - 1)])
    # a probe of the padding mode at the left edge: pixel (0, 14) of frame 1 reads fflow[0] half a pixel outside the image (zero
    # padding: cycle error 0.5, border padding: 1.5), it is hit, and the trajectory of (0, 15) passes through it (0.5 rounds to 0),
    # so that it starts a trajectory at frame 1 only if its cycle error is wrong
    fflow[0][:, 14, 0] = (2.0, 0.0)
    fflow[0][:, 15, 0] = (0.5, -1.0)
    bflow[0][:, 14, 0] = (-0.5, 0.0)
    bflow[0][:, 14, 1] = (-0.5, 2.0)
    fflow[1][:, 14, 0] = (1.0, 0.0)    # (such a trajectory lives on: plain background motion behind the probe)
    bflow[1][:, 14, 1] = (-1.0, 0.0)
    direct = []
    for s in range(T - 1):
        fwd = np.stack([field(_rect(s, h, w), (-2, 1), (1, 0), k + 1, 8, 2.0) for k in range(T - 1 - s)])
        back = np.stack([field(_rect(s + k + 1, h, w), (2, -1), (-1, 0), k + 1, 10, -2.0) for k in range(T - 1 - s)])
        direct.append((fwd.astype(np.float32), back.astype(np.float32)))
    return dict(T=T, h=h, w=w, fflow=fflow.astype(np.float32), bflow=bflow.astype(np.float32), direct=direct)


# ---- smooth ---------------------------------------------------------------------------------------------------------------------
def _affine(rng, h, w):
    """a small rotation-zoom-shear about the image centre plus a shift of a few pixels: (a, b, tx, c, d, ty) with
    x' = a x + b y + tx, y' = c x + d y + ty (plain scalar arithmetic: no BLAS call whose summation order could differ)"""
    e = (rng.random(4) - 0.5) * 0.06
    a, b, c, d = 1.0 + float(e[0]), float(e[1]), float(e[2]), 1.0 + float(e[3])
    cx, cy = (w - 1) / 2, (h - 1) / 2
    t = rng.random(2) - 0.5
    return (a, b, cx - (a * cx + b * cy) + float(t[0]) * 6.0, c, d, cy - (c * cx + d * cy) + float(t[1]) * 4.0)


def _compose(q, p):
    """q after p"""
    a, b, tx, c, d, ty = p
    A, B, TX, C, D, TY = q
    return (A * a + B * c, A * b + B * d, A * tx + B * ty + TX, C * a + D * c, C * b + D * d, C * tx + D * ty + TY)


def _invert(p):
    a, b, tx, c, d, ty = p
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    return (ia, ib, -(ia * tx + ib * ty), ic, id_, -(ic * tx + id_ * ty))


def _flow_of(p, h, w):
    xx, yy = _grid(h, w)
    a, b, tx, c, d, ty = p
    return np.stack([a * xx + b * yy + tx - xx, c * xx + d * yy + ty - yy])


def smooth(seed=SMOOTH["seed"], T=SMOOTH["T"], h=SMOOTH["h"], w=SMOOTH["w"]):
    rng = np.random.default_rng(seed)
    xx, yy = _grid(h, w)
    cx, cy, r = 0.3 * w, 0.55 * h, 0.16 * min(h, w)
    disc = ((xx - cx) * (xx - cx) + (yy - cy) * (yy - cy) < r * r)

    def noise():
        n = (rng.random((2, h, w)) - 0.5) * 0.3   # +-0.15 px
        return np.where(disc, 12.0 * n, n)

    maps = [_affine(rng, h, w) for _ in range(T - 1)]
    fflow = np.stack([_flow_of(m, h, w) + noise() for m in maps])
    bflow = np.stack([_flow_of(_invert(m), h, w) + noise() for m in maps])
    right = (xx > 0.6 * w).astype(np.float64)
    direct = []
    for s in range(T - 1):
        fwd, back = [], []
        acc = None
        for k in range(T - 1 - s):
            acc = maps[s + k] if acc is None else _compose(maps[s + k], acc)
            drift = np.stack([0.45 * (k + 1) * right, -0.2 * (k + 1) * right])
            fwd.append(_flow_of(acc, h, w) + noise() + drift)
            back.append(_flow_of(_invert(acc), h, w) + noise() - drift)
        direct.append((np.stack(fwd).astype(np.float32), np.stack(back).astype(np.float32)))
    return dict(T=T, h=h, w=w, fflow=fflow.astype(np.float32), bflow=bflow.astype(np.float32), direct=direct)


def outward(T=4, h=19, w=27):
    """every pixel is pushed out of the image at once: no trajectory survives a single step"""
    f = np.zeros((T - 1, 2, h, w), dtype=np.float32)
    f[:, 0] = 3.0 * w
    return dict(T=T, h=h, w=w, fflow=f, bflow=-f, direct=[(f[s:].copy(), -f[s:]) for s in range(T - 1)])


# name -> (case maker, min_trajectory_length): the cases of the golden file; each runs with and without the direct filter
GOLDEN_CASES = {"lattice": (lattice, 2), "lattice_min3": (lattice, 3), "smooth": (smooth, 2)}
