"""Seeded inputs of the PCA foreground-mask fixtures (tests/golden/fg_mask.npz, written by make_golden_fgmask.py).

Everything here is integer arithmetic or IEEE +, -, *, / on numpy arrays (no transcendental functions), so the arrays are
bit-identical on every machine; fg_mask.npz pins their sha256 digests and the tests check them before comparing outputs.

`features(case)` -- DINO-like features [T, C, h, w] float32: a common offset vector (unit-norm DINO rows share a large mean), a
background direction, a foreground direction on a soft elliptical blob that covers about a fifth of the grid and moves from
frame to frame, and per-token noise.  The blob stays clear of the border of the grid.
"""
import hashlib

import numpy as np

# case -> (T, C, h, w)
CASES = {"A": (3, 384, 15, 29), "B": (2, 1024, 11, 13), "C": (3, 768, 15, 29)}
# the image size of the stored upsampled mask
IMG_SIZE = {"A": (112, 210), "B": (90, 101), "C": (111, 209)}
SEEDS = {"A": 3841529, "B": 10241113, "C": 7681529}
THRESHOLDS = (0.4, 0.6)
NOISE = 0.6


def digest(a: np.ndarray) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def blob_weight(case: str) -> np.ndarray:
    """[T, h, w] float64 in (0, 1]: 1 / (1 + d^6) of the elliptical distance d to the frame's blob centre."""
    T, _, h, w = CASES[case]
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = np.empty((T, h, w), dtype=np.float64)
    for t in range(T):
        cx, cy = (w - 1) * (0.4 + 0.1 * t), (h - 1) * (0.45 + 0.05 * t)
        rx, ry = 0.25 * w, 0.25 * h
        d2 = ((xx - cx) / rx) * ((xx - cx) / rx) + ((yy - cy) / ry) * ((yy - cy) / ry)
        out[t] = 1.0 / (1.0 + d2 * d2 * d2)
    return out


def features(case: str) -> np.ndarray:
    T, C, h, w = CASES[case]
    rng = np.random.default_rng(SEEDS[case])
    offset = rng.uniform(-1.0, 1.0, size=C) * 1.5
    bg = rng.uniform(-1.0, 1.0, size=C)
    fg = rng.uniform(-1.0, 1.0, size=C)
    s = blob_weight(case)[:, None]                                         # [T, 1, h, w]
    noise = rng.uniform(-1.0, 1.0, size=(T, C, h, w)) * NOISE
    c = lambda v: v[None, :, None, None]  # noqa: E731
    return (c(offset) + (1.0 - s) * c(bg) + s * c(fg) + noise).astype(np.float32)


def blob_tokens(case: str) -> np.ndarray:
    """[T, h, w] bool: the tokens well inside the blob (weight > 0.9)."""
    return blob_weight(case) > 0.9
