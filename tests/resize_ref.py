"""numpy restatement of Pillow's 8-bit LANCZOS resize (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
ImagingResampleHorizontal_8bpc / Vertical_8bpc), the yardstick of the device resize where Pillow is absent.  It is checked against
live Pillow and against Pillow's committed outputs (tests/golden/resize_lanczos.npz) in tests/test_resize_reference.py.

Also the case list the golden file, the CPU tests and the GPU tests share; inputs are regenerated from a seed, never stored."""
import math

import numpy as np

PRECISION_BITS = 22


def lanczos(x):
    if not (-3.0 <= x < 3.0):
        return 0.0
    if x == 0.0:
        return 1.0
    a, b = x * math.pi, x / 3 * math.pi
    return (math.sin(a) / a) * (math.sin(b) / b)


def tables(in_size, out_size):
    """(k int64 [out, ksize], bounds int64 [out, 2]) as precompute_coeffs + normalize_coeffs_8bpc build them (Python floats are C
    doubles, math.sin is libm's).  Raises if a row could overflow the int32 accumulator or a weight the 24-bit multiply."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    k = np.zeros((out_size, ksize), dtype=np.int64)
    bounds = np.zeros((out_size, 2), dtype=np.int64)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = [lanczos((j + xmin - center + 0.5) * (1.0 / fs)) for j in range(xmax - xmin)]
        total = 0.0
        for v in w:
            total += v
        for j, v in enumerate(w):
            v = v / total if total != 0.0 else v
            k[i, j] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
        bounds[i] = (xmin, xmax - xmin)
    if not (np.abs(k).max() < (1 << 23) and (255 * np.abs(k).sum(axis=1) + (1 << 21)).max() < (1 << 31)):
        raise OverflowError(f"lanczos tables {in_size} -> {out_size} overflow the int32 accumulator")
    return k, bounds


def one_pass(a, k, bounds, axis):
    """acc = 2^21 + sum_j a[first + j] k[j] along `axis`, out = clamp(acc >> 22, 0, 255); uint8 in, uint8 out."""
    a = np.moveaxis(a, axis, -1).astype(np.int64)
    n_in, ksize = a.shape[-1], k.shape[1]
    idx = np.minimum(bounds[:, :1] + np.arange(ksize)[None], n_in - 1)          # [out, ksize]; weights beyond count are 0
    live = np.arange(ksize)[None] < bounds[:, 1:]
    acc = (1 << (PRECISION_BITS - 1)) + (a[..., idx] * np.where(live, k, 0)).sum(-1)
    assert acc.min() >= -(1 << 31) and acc.max() < (1 << 31)
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, -1, axis)


def resize(frames, h, w):
    """uint8 [N, H, W, C] -> uint8 [N, h, w, C]: horizontal pass, then vertical pass on its uint8 result; a pass whose size does not
    change is skipped."""
    assert frames.dtype == np.uint8 and frames.ndim == 4
    H, W = frames.shape[1:3]
    out = frames
    if W != w:
        out = one_pass(out, *tables(W, w), axis=2)
    if H != h:
        out = one_pass(out, *tables(H, h), axis=1)
    return np.ascontiguousarray(out)


def to_tensor(u8_nhwc):
    """ToTensor: uint8 [N, h, w, C] -> float32 [N, C, h, w] = u8 / 255 (one correctly rounded fp32 division)."""
    return np.ascontiguousarray(u8_nhwc.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)


# (name, N, H, W, C, h, w) -- tests/test_gpu_video_io.py says what each is for.  The device kernel's tile is 32 x 64 output pixels.
CASES = (
    ("down_rgb", 1, 37, 53, 3, 16, 24),
    ("up_rgb", 1, 16, 24, 3, 37, 53),
    ("v_only", 1, 40, 64, 3, 36, 64),
    ("h_only", 1, 40, 64, 3, 40, 31),
    ("ksize259", 1, 20, 300, 3, 19, 7),
    ("to_1x1", 1, 7, 5, 3, 1, 1),
    ("from_1x1", 1, 1, 1, 3, 9, 4),
    ("mode_l", 1, 41, 29, 1, 17, 13),
    ("frames3", 3, 37, 53, 3, 16, 24),
    ("multi_tile", 1, 70, 131, 3, 45, 83),
    ("tall", 1, 400, 8, 3, 3, 5),
    ("same_size", 1, 12, 10, 3, 12, 10),
)
CONTENTS = ("uniform", "binary")


def case_input(name, content):
    """The seeded input of a case: uniform random bytes, or random {0, 255} pixels (the accumulator passes both clamps)."""
    i = [c[0] for c in CASES].index(name)
    _, N, H, W, C, _, _ = CASES[i]
    rng = np.random.default_rng([20251, i, CONTENTS.index(content)])
    if content == "uniform":
        return rng.integers(0, 256, size=(N, H, W, C), dtype=np.uint8)
    return (rng.integers(0, 2, size=(N, H, W, C), dtype=np.uint8) * 255).astype(np.uint8)


def all_cases():
    return [(c, content) for c in CASES for content in CONTENTS]
