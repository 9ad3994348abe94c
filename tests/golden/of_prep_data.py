"""Seeded inputs of the optical-flow preprocessing fixtures (tests/golden/of_prep.npz, written by make_golden_of.py).

Everything here is integer arithmetic or IEEE +, -, *, / on numpy arrays (no transcendental functions), so the arrays are
bit-identical on every machine; of_prep.npz pins their sha256 digests and the tests check them before comparing outputs.

* `filter_trajectories()` -- T = 8 frames of 112 x 210 px, ~20 k trajectories that start on integer pixels at several frames,
  move with a smooth random (polynomial) flow and end at random; frame EMPTY_FRAME has no tracked point, and TIE_GROUPS groups
  of three rows sit exactly on one grid point at one frame (exact ties: the lowest row must win).
* `split_trajectories()` -- ~20 k trajectories over the same 8 frames in 476 x 854 px (the resolution load_masks resizes to);
  a tenth of them start on half-integers (torch.round is half-to-even).
* `mask_frames()` -- 8 blob masks at 119 x 214 (0 / 255), written as PNGs by `write_masks`.
* `bb_features()` -- the DINO features the best buddies are extracted from (dino_tracker_amd.synth).
"""
import hashlib
import os

import numpy as np

T, H, W = 8, 112, 210
STRIDE = 7
C = 32
EMPTY_FRAME = 5
TIE_GROUPS = 24
SPLIT_H, SPLIT_W = 476, 854
MASK_H, MASK_W = 119, 214
N_FILTER, N_SPLIT = 20000, 20000


def digest(a: np.ndarray) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def _flow_coeffs(rng, h, w, scale):
    # per frame: u, v = a0 + a1 x' + a2 y' + a3 x' y' with x' = x / w, y' = y / h  (px per frame)
    return rng.uniform(-scale, scale, size=(T, 2, 4))


def _advect(rng, n, h, w, scale, half_frac=0.0):
    """n trajectories [n, T, 2] float32: integer start pixel (a fraction on half-integers) at a random frame, then the flow,
    NaN before the start and after a random end."""
    coef = _flow_coeffs(rng, h, w, scale)
    s0 = rng.integers(0, T - 1, size=n)
    length = 2 + (rng.integers(0, 1 << 30, size=n) % (T - s0)).astype(np.int64)
    end = np.minimum(s0 + length - 1, T - 1)
    x = rng.integers(0, w - 1, size=n).astype(np.float64)
    y = rng.integers(0, h - 1, size=n).astype(np.float64)
    half = rng.uniform(size=n) < half_frac
    x[half] += 0.5
    y[half & (rng.uniform(size=n) < 0.5)] += 0.5
    out = np.full((n, T, 2), np.nan, dtype=np.float32)
    px, py = x.copy(), y.copy()
    for t in range(T):
        live = (t >= s0) & (t <= end)
        out[live, t, 0] = px[live]
        out[live, t, 1] = py[live]
        a = coef[t]
        xs, ys = px / w, py / h
        u = a[0, 0] + a[0, 1] * xs + a[0, 2] * ys + a[0, 3] * xs * ys
        v = a[1, 0] + a[1, 1] * xs + a[1, 2] * ys + a[1, 3] * xs * ys
        moving = t >= s0
        px = np.where(moving, px + u, px)
        py = np.where(moving, py + v, py)
    return out


def grid_points(h=H, w=W, stride=STRIDE):
    xs = np.arange(7, w, stride, dtype=np.float32)
    ys = np.arange(7, h, stride, dtype=np.float32)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    return np.stack([xx.reshape(-1), yy.reshape(-1)], axis=-1)


def _filter_case():
    rng = np.random.default_rng(20261016)
    traj = _advect(rng, N_FILTER, H, W, 3.0)
    traj[:, EMPTY_FRAME] = np.nan
    grid = grid_points()
    rows = rng.permutation(N_FILTER)[:3 * TIE_GROUPS].reshape(TIE_GROUPS, 3)
    ties = []
    for k in range(TIE_GROUPS):
        t = int(rng.integers(0, T))
        t = t if t != EMPTY_FRAME else t + 1
        gi = int(rng.integers(0, grid.shape[0]))
        traj[rows[k], t] = grid[gi]
        ties.append((rows[k], t, gi))
    return traj, ties


def filter_trajectories() -> np.ndarray:
    return _filter_case()[0]


def tie_rows():
    """[(rows [3], frame, grid index)] of the hand-placed exact ties: three rows exactly on one grid point at one frame."""
    return _filter_case()[1]


def split_trajectories() -> np.ndarray:
    rng = np.random.default_rng(4761854)
    return _advect(rng, N_SPLIT, SPLIT_H, SPLIT_W, 12.0, half_frac=0.1)


def mask_frames() -> np.ndarray:
    rng = np.random.default_rng(119214)
    yy, xx = np.meshgrid(np.arange(MASK_H, dtype=np.float64), np.arange(MASK_W, dtype=np.float64), indexing="ij")
    m = np.zeros((T, MASK_H, MASK_W), dtype=np.uint8)
    for t in range(T):
        for _ in range(4):
            cx, cy = rng.uniform(0, MASK_W), rng.uniform(0, MASK_H)
            rx, ry = rng.uniform(10, 50), rng.uniform(8, 35)
            inside = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0
            m[t][inside] = 255
    return m


def write_masks(folder: str) -> str:
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for t, m in enumerate(mask_frames()):
        Image.fromarray(m).save(os.path.join(folder, f"{t:05d}.png"))
    return folder


def bb_features():
    from dino_tracker_amd import synth
    ph, pw = 1 + (H - 14) // STRIDE, 1 + (W - 14) // STRIDE
    return synth.synth_features(T, C, ph, pw, seed=77)


def nms_pair(s: int, t: int) -> bool:
    """The pairs that carry compute_dino_bb_nms's keys (peak_coords / peak_affs / r) into the filter: half of them."""
    return t % 2 == 0
