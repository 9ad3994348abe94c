"""The JPEG files the sampling tests share (CPU: tests/test_jpeg_sampling_reference.py, GPU: tests/test_gpu_jpeg_sampling.py): one
picture written by Pillow as gray, 4:4:4, 4:2:2 or 4:2:0 in its four stream variants, the same with an Adobe APP14 segment spliced
in, and DAMAGED single-segment files per sampling (tests/jpeg_dec_cases.py's recipe: cut in the middle of the scan; sixteen 1-bits,
which no code of the Annex K tables matches, at its start)."""
import functools
import io

import numpy as np

import jpeg_dec_cases as C
import jpeg_ref as J
import jpeg_sampling_ref as R

SAMPLINGS = (R.GRAY, R.S444, R.S422, R.S420)
_PILLOW_SUBSAMPLING = {R.S444: 0, R.S422: 1, R.S420: 2}


def picture(kind, h, w, sampling, seed=0):
    """uint8 [h, w, 3], for GRAY uint8 [h, w] (the picture's green channel)"""
    img = J.picture(kind, h, w, seed=seed)
    return np.ascontiguousarray(img[..., 1]) if sampling == R.GRAY else img


def encode(img, sampling, quality, **kw):
    from PIL import Image
    buf = io.BytesIO()
    if sampling != R.GRAY:
        kw = dict(kw, subsampling=_PILLOW_SUBSAMPLING[sampling])
    Image.fromarray(img).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def pillow_decode(data):
    """uint8 [H, W, 3], or [H, W] for a gray file"""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:
        assert img.mode in ("RGB", "L"), img.mode
        return np.asarray(img).copy()


def variants(img, sampling, quality):
    """(name, file): Pillow's encoder with its defaults, optimize=True, restart_marker_blocks=3, restart_marker_rows=1"""
    return [(name, encode(img, sampling, quality, **kw)) for name, kw in C.PILLOW_VARIANTS]


def with_adobe(data, transform=1, keep_jfif=True):
    """the file with FF EE 00 0E "Adobe" 00 64 00 00 00 00 <transform> after SOI (or in the JFIF segment's place)"""
    seg = b"\xff\xee\x00\x0e" + b"Adobe" + bytes([0, 100, 0, 0, 0, 0, transform])
    if keep_jfif:
        return data[:2] + seg + data[2:]
    assert data[2:4] == b"\xff\xe0", "no JFIF segment to replace"
    return data[:2] + seg + data[4 + int.from_bytes(data[4:6], "big"):]


def gray_with_factors(data, factors=0x22):
    """a gray file whose SOF names other sampling factors: the single-component scan is one block per MCU all the same"""
    at = data.index(b"\xff\xc0")
    assert data[at + 9] == 1 and data[at + 11] == 0x11
    return data[:at + 11] + bytes([factors]) + data[at + 12:]


def sof_factors_patched(data, factors):
    """a three-component file with the first component's sampling factors overwritten (4:4:4 -> 0x12: the header of a 4:4:0 file)"""
    at = data.index(b"\xff\xc0")
    assert data[at + 9] == 3
    return data[:at + 11] + bytes([factors]) + data[at + 12:]


DAMAGED_SIZE = (31, 47)
STATUS = {"truncated": C.S_OVERRUN, "unknown_code": C.S_CODE}


def good_file(sampling, seed=0):
    """one segment (no restart markers), the Annex K tables"""
    return encode(picture("noise", *DAMAGED_SIZE, sampling, seed=seed), sampling, 90)


@functools.lru_cache(maxsize=None)
def damaged(sampling):
    data = good_file(sampling)
    s = C.scan_start(data)
    n = len(data) - 2 - s
    return [("truncated", data[:s + n // 2]), ("unknown_code", data[:s] + b"\xff\x00\xff\x00" + data[s + 4:])]
