"""The JPEG files the decoder tests share (CPU: tests/test_jpeg_decode_reference.py, GPU: tests/test_gpu_jpeg_decode.py): stream
variants of one picture, and a handful of DAMAGED files.  The damaged ones are single-segment files (6 MCUs, fewer than the
restart interval), so a frame's status is its segment's; the CPU test runs exactly these through the stand-alone sanitiser program
(tests/host/jpeg_entropy_host.cpp) and holds it to STATUS below, the GPU test holds the device to the same values."""
import functools
import io
import struct

import numpy as np

import jpeg_ref as J

S_CODE, S_INDEX, S_OVERRUN, S_LEFTOVER, S_RANGE, S_SEGMENT = 1, 2, 4, 8, 16, 32

PILLOW_VARIANTS = (("pillow", {}), ("pillow_optimize", {"optimize": True}), ("pillow_rst_blocks3", {"restart_marker_blocks": 3}),
                   ("pillow_rst_rows1", {"restart_marker_rows": 1}))


def pillow_encode(img, quality, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:
        assert img.mode == "RGB", img.mode
        return np.asarray(img).copy()


def variants(img, quality):
    """(name, file) of one picture: the restatement's encoder at R = 1, 3, 16 and Pillow's encoder in four settings"""
    out = [(f"ref_R{R}", J.encode(img, quality, R)) for R in (1, 3, 16)]
    return out + [(name, pillow_encode(img, quality, **kw)) for name, kw in PILLOW_VARIANTS]


def scan_start(data):
    """index of the first entropy-coded byte"""
    i = 2
    while True:
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        i += 2 + length
        if marker == 0xDA:
            return i


DAMAGED_SIZE = (31, 47)


def good_file(seed=0):
    return J.encode(J.picture("noise", *DAMAGED_SIZE, seed=seed), 90, J.RESTART)


@functools.lru_cache(maxsize=None)
def damaged():
    """[(name, file)]: the good file cut in the middle of its scan (no EOI), with one bit of its scan flipped, and with sixteen
    1-bits -- which no code of the Annex K tables matches -- at the start of its scan"""
    data = good_file()
    s = scan_start(data)
    n = len(data) - 2 - s
    # A flipped VALUE bit only changes a coefficient: that is no damage anybody can see.  Take the first byte from a third of the scan
    # on whose flip the RESTATEMENT finds damaged (a code that ends elsewhere: the stream falls out of step) and that neither makes
    # nor breaks a marker.
    import jpeg_dec_ref as D
    for at in range(s + n // 3, s + n):
        flipped = bytearray(data)
        flipped[at] ^= 0x10
        if 0xFF in (data[at - 1], data[at], data[at + 1], flipped[at]) or 0x00 in (data[at], flipped[at]):
            continue
        info = {}
        try:
            D.coefficients(bytes(flipped), info=info)
        except AssertionError:
            info["damaged"] = True
        if info["damaged"]:
            break
    else:
        raise AssertionError("no flip damages the stream")
    return [("truncated", data[:s + n // 2]),
            ("flipped_bit", bytes(flipped)),
            ("unknown_code", data[:s] + b"\xff\x00\xff\x00" + data[s + 4:])]


# what the stand-alone host program reports for damaged()'s files (and the device must): asserted by the CPU test
STATUS = {"truncated": S_OVERRUN, "unknown_code": S_CODE}


def case_file(data):
    """the host program's input for a single-segment file: 6 raw tables, int32 MCU count, the segment's bytes"""
    from dino_tracker_amd import video_in
    h, why = video_in.parse_jpeg(data)
    assert h is not None and h.segments.shape[0] == 1, why
    off, length, _, count = (int(v) for v in h.segments[0])
    return h.huffman.tobytes() + struct.pack("<i", count) + bytes(data[off:off + length])
