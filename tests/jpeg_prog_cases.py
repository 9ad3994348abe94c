"""The progressive JPEG files the progressive tests share (CPU: tests/test_jpeg_progressive_reference.py, GPU:
tests/test_gpu_jpeg_progressive.py): one picture written by Pillow as a baseline and as a progressive file with the same settings --
the oracle is *progressive coefficients = baseline coefficients* --, the flat picture whose end-of-band runs reach category 14, the
real frame re-encoded, files edited into what the parser must refuse, damaged files, and the case files of the stand-alone host
program (tests/host/jpeg_progressive_host.cpp)."""
import functools
import io
import os
import struct

import numpy as np

import jpeg_prog_ref as P
import jpeg_sampling_cases as SC
import jpeg_sampling_ref as R

SAMPLINGS = SC.SAMPLINGS                     # gray, 4:4:4, 4:2:2, 4:2:0
RESTARTS = (("none", {}), ("blocks3", {"restart_marker_blocks": 3}), ("rows1", {"restart_marker_rows": 1}))
HORSEJUMP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "horsejump_00000.jpg")
S_CODE, S_INDEX, S_OVERRUN, S_LEFTOVER, S_RANGE, S_SEGMENT = 1, 2, 4, 8, 16, 32
picture, pillow_decode = SC.picture, SC.pillow_decode


def encode(img, sampling, quality, progressive=True, **kw):
    """Pillow's file of `img` (SC.picture's layout); progressive files may outgrow Pillow's default encoder buffer"""
    from PIL import ImageFile
    if progressive:
        kw = dict(kw, progressive=True)
    saved = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(saved, 4 * img.size + (1 << 16))
    try:
        return SC.encode(img, sampling, quality, **kw)
    finally:
        ImageFile.MAXBLOCK = saved


@functools.lru_cache(maxsize=None)
def pair(kind, h, w, sampling, quality, restart="none", seed=0):
    """(baseline file, progressive file) of one picture and one set of settings"""
    img = picture(kind, h, w, sampling, seed=seed)
    kw = dict(RESTARTS)[restart]
    return encode(img, sampling, quality, progressive=False, **kw), encode(img, sampling, quality, **kw)


@functools.lru_cache(maxsize=None)
def flat_file():
    """gray 1024 x 1024, flat but for one pixel: 4.4 kB whose first and refinement scans hold end-of-band runs up to category 14"""
    img = np.full((1024, 1024), 128, np.uint8)
    img[517, 300] = 160
    return encode(img, R.GRAY, 75)


@functools.lru_cache(maxsize=None)
def real_frame():
    """the 854 x 480 frame of tests/golden re-encoded as a progressive file (4:2:0, quality 90, no restart markers)"""
    from PIL import Image
    with Image.open(HORSEJUMP) as img:
        return encode(np.asarray(img.convert("RGB")), R.S420, 90)


def scan_offsets(data):
    """the byte offset of every SOS marker of a file, by walking its segments"""
    out, i = [], 2
    while data[i + 1] != 0xD9:
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if marker == 0xDA:
            out.append(i)
            i += 2 + length
            while not (data[i] == 0xFF and data[i + 1] != 0 and not 0xD0 <= data[i + 1] <= 0xD7):
                i += 1
        else:
            i += 2 + length
    return out


def cut_after_scans(data, n):
    """the first n scans, then EOI: an incomplete progression"""
    at = scan_offsets(data)[n]
    while data[at - 1:at + 1] != b"\xff\xda":      # back over the DHT in front of that scan
        at -= 1
    end = at - 1
    i, last = 2, 2
    while i < end:                                   # the start of the segment (DHT ...) that precedes scan n
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if marker == 0xDA:
            i += 2 + length
            while not (data[i] == 0xFF and data[i + 1] != 0 and not 0xD0 <= data[i + 1] <= 0xD7):
                i += 1
            last = i
        else:
            i += 2 + length
    return data[:last] + b"\xff\xd9"


def with_scan_bits(data, n, ah, al):
    """scan n's Ah/Al byte overwritten"""
    at = scan_offsets(data)[n]
    length = int.from_bytes(data[at + 2:at + 4], "big")
    return data[:at + 1 + length] + bytes([(ah << 4) | al]) + data[at + 2 + length:]


def dqt_behind_first_scan(data):
    """the first DQT segment moved behind the first scan's body"""
    at = data.index(b"\xff\xdb")
    length = int.from_bytes(data[at + 2:at + 4], "big")
    dqt, rest = data[at:at + 2 + length], data[:at] + data[at + 2 + length:]
    second = scan_offsets(rest)[1]
    i, last = 2, 2
    while i < second:                                # the first segment behind scan 0's body
        marker, n = rest[i + 1], int.from_bytes(rest[i + 2:i + 4], "big")
        i += 2 + n
        if marker == 0xDA:
            while not (rest[i] == 0xFF and rest[i + 1] != 0 and not 0xD0 <= rest[i + 1] <= 0xD7):
                i += 1
            last = i
            break
    return rest[:last] + dqt + rest[last:]


def sof_factors_patched(data, factors):
    """a three-component progressive file with the first component's sampling factors overwritten (0x12: a 4:4:0 header)"""
    at = data.index(b"\xff\xc2")
    assert data[at + 9] == 3
    return data[:at + 11] + bytes([factors]) + data[at + 12:]


DAMAGED_SIZE = (31, 47)
STATUS = {"truncated": S_OVERRUN, "unknown_code": S_CODE}


def good_file(sampling=R.S420, seed=0):
    return encode(picture("noise", *DAMAGED_SIZE, sampling, seed=seed), sampling, 90)


@functools.lru_cache(maxsize=None)
def damaged(sampling=R.S420):
    """(name, file): the LAST scan's body (the luma refinement 1-63 to Al = 0, which no other scan builds on, so the frame's status is
    this scan's alone) cut to its first half, and the same body with sixteen 1-bits at its start, which no code of an optimised table
    matches (the all-ones code is reserved).  Both keep a header and a scan script the parser accepts."""
    data = good_file(sampling)
    last = scan_offsets(data)[-1]
    body = last + 2 + int.from_bytes(data[last + 2:last + 4], "big")
    end = len(data) - 2
    assert data[end:] == b"\xff\xd9"
    half = body + (end - body) // 2
    if data[half - 1] == 0xFF:
        half -= 1
    return [("truncated", data[:half] + data[end:]), ("unknown_code", data[:body] + b"\xff\x00\xff\x00" + data[body + 4:])]


def case_file(data):
    """what tests/host/jpeg_progressive_host.cpp reads: int64 magic, sampling, H, W, rows, tables, stream bytes; the rows
    (video_in.plan_jpeg_progressive's); the raw tables; the file; the restatement's coefficients"""
    from dino_tracker_amd import video_in
    plan, why = video_in.plan_jpeg_progressive([data])
    assert plan is not None, why
    want = P.coefficients(data)
    head = struct.pack("<7q", 0x50524F47, plan.sampling, plan.height, plan.width, plan.segments.shape[0], plan.tables.shape[0], len(data))
    return head + plan.segments.astype("<i8").tobytes() + plan.tables.tobytes() + bytes(data) + want.astype("<i2").tobytes()
