"""Video output without imageio, cv2 or ffmpeg: rendered frames leave the device as baseline JPEG files (csrc/jpeg.hip, arithmetic
in docs/JPEG.md) and are written as a Motion-JPEG AVI or as a folder of 00000.jpg ... frames.

    encode_jpeg(frames, quality)              device uint8 [F, H, W, 3] -> (device uint8 [bytes], int64 [F + 1] offsets)
    write_mjpeg_avi(frames, path, fps)        RIFF AVI: hdrl (avih, strl: strh vids / MJPG, strf BITMAPINFOHEADER), movi of 00dc
                                              chunks -- one whole JPEG file each --, idx1
    write_jpeg_frames(frames, folder)         00000.jpg ..., the names load_video and the reference's loaders glob
    read_mjpeg_avi(path)                      the strict inverse of write_mjpeg_avi: the JPEG byte strings, or with device=...
                                              the frames decoded on the device (video_in.py)

The host builds what does not depend on the pixels: the quantisation tables of a quality (quant_tables) and the file header SOI ..
SOS (jpeg_header).  Everything per pixel runs on the device; there is no CPU encoder here -- CPU tensors are refused, numpy
arrays are uploaded.  The AVI is checked by read_mjpeg_avi and its frames by Pillow's decoder; no media player or ffmpeg was
available where this was written, so it has not been played (docs/JPEG.md section 9)."""
from __future__ import annotations

import os
import struct
from typing import Callable, Iterable, Iterator, List, Optional, Tuple

import numpy as np
import torch

RESTART = 16                         # MCUs per restart interval (DTK_JPEG_RESTART)
AVI_LIMIT = 1 << 30                  # a RIFF AVI without OpenDML extensions; files that would reach it are refused
WORKSPACE_BUDGET = 256 << 20         # device bytes of one batch's workspace (about 13 bytes per pixel, docs/JPEG.md section 7)
WORST_CASE_LIMIT = 64 << 20          # output buffers up to this size are allocated at the worst-case bound: no retry can happen
GUESS_BYTES_PER_PIXEL = 0.75         # beyond it: a guess (a noisy quality-90 render measured 0.4), and one retry when it is short

# natural (row-major) position of the k-th zigzag coefficient
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# ITU-T T.81 Annex K.1, natural order
_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
              80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
              95, 98, 112, 100, 103, 99)
_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                99, 99, 99) + (99,) * 32
# ITU-T T.81 Annex K.3: DHT payloads (table class and id, 16 counts, the symbols) of the four typical tables
_DC_COUNTS_LUMA = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
_DC_COUNTS_CHROMA = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
_AC_COUNTS_LUMA = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D)
_AC_COUNTS_CHROMA = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)
_AC_SYMBOLS_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_SYMBOLS_CHROMA = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
    "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN_TABLES = ((0x00, _DC_COUNTS_LUMA, bytes(range(12))), (0x10, _AC_COUNTS_LUMA, _AC_SYMBOLS_LUMA),
                  (0x01, _DC_COUNTS_CHROMA, bytes(range(12))), (0x11, _AC_COUNTS_CHROMA, _AC_SYMBOLS_CHROMA))


# ---- host: tables and header ---------------------------------------------------------------------------------------------------
def quant_tables(quality: int) -> np.ndarray:
    """uint8 [2, 64]: the luma and the chroma table of `quality` (1 .. 100) in zigzag order, as a DQT segment stores them and as
    dtk_jpeg_encode reads them.  scale = 5000 / q below 50, else 200 - 2 q;  Q = clamp((base * scale + 50) / 100, 1, 255)."""
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError(f"quant_tables: quality must be an integer in 1 .. 100, got {quality!r}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    out = np.empty((2, 64), dtype=np.uint8)
    for row, base in enumerate((_BASE_LUMA, _BASE_CHROMA)):
        out[row] = [min(255, max(1, (base[n] * scale + 50) // 100)) for n in ZIGZAG]
    return out


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes((0xFF, marker)) + struct.pack(">H", len(payload) + 2) + payload


def jpeg_header(h: int, w: int, quality: int) -> bytes:
    """SOI, APP0 JFIF 1.01 (no units, 1 : 1), DQT x 2, SOF0 (Y 2 x 2, Cb, Cr 1 x 1), DHT x 4, DRI, SOS: everything in front of
    the entropy-coded segment of an h x w frame."""
    h, w = int(h), int(w)
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"jpeg_header: a frame must be 1 .. 65535 pixels each way, got {h} x {w}")
    q = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes((1, 1, 0, 0, 1, 0, 1, 0, 0)))
    out += _segment(0xDB, b"\0" + q[0].tobytes()) + _segment(0xDB, b"\1" + q[1].tobytes())
    out += _segment(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for ident, counts, symbols in HUFFMAN_TABLES:
        out += _segment(0xC4, bytes((ident,)) + bytes(counts) + symbols)
    out += _segment(0xDD, struct.pack(">H", RESTART))
    return out + _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


# ---- device: frames -> JPEG files ----------------------------------------------------------------------------------------------
def _device_frames(frames) -> torch.Tensor:
    if isinstance(frames, torch.Tensor):
        if not frames.is_cuda:
            raise RuntimeError("dino_tracker_amd: tensor is not on a GPU -- the hot path has no CPU fallback")
        t = frames
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(frames))).to("cuda:0")
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or t.numel() == 0:
        raise TypeError(f"frames must be uint8 [F, H, W, 3] with F, H, W >= 1, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def frames_per_batch(F: int, H: int, W: int, budget: Optional[int] = None) -> int:
    """frames of one dtk_jpeg_encode call: as many as keep its workspace inside `budget` (WORKSPACE_BUDGET) bytes, at least one"""
    from . import ops
    budget = WORKSPACE_BUDGET if budget is None else int(budget)
    return max(1, min(int(F), budget // max(1, ops.jpeg_workspace_bytes(1, H, W))))


def first_capacity(F: int, H: int, W: int, header_bytes: int) -> int:
    """The capacity policy (docs/JPEG.md section 7): the worst-case bound where that is small, else header + 0.75 bytes per pixel
    per frame -- the call reports the needed size when that is short, and ops.jpeg_encode retries once."""
    from . import ops
    worst = ops.jpeg_worst_case_bytes(F, H, W, header_bytes)
    if worst <= WORST_CASE_LIMIT:
        return worst
    return min(worst, F * (header_bytes + int(GUESS_BYTES_PER_PIXEL * H * W) + 4096))


def _batches(frames: torch.Tensor, quality: int) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
    from . import ops
    F, H, W = (int(v) for v in frames.shape[:3])
    head = jpeg_header(H, W, quality)
    header = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(frames.device)
    qt = torch.from_numpy(quant_tables(quality)).to(frames.device)
    step = frames_per_batch(F, H, W)
    for f0 in range(0, F, step):
        part = frames[f0:f0 + step]
        yield ops.jpeg_encode(part, qt, header, first_capacity(int(part.shape[0]), H, W, len(head)))


def encode_jpeg(frames, quality: int = 90) -> Tuple[torch.Tensor, torch.Tensor]:
    """frames uint8 [F, H, W, 3] on the device -> (uint8 [bytes], int64 [F + 1]), both on the device: file f is
    bytes[offsets[f] : offsets[f + 1]], a complete baseline JPEG (4:2:0, restart interval 16).  Frames are encoded in batches sized
    to WORKSPACE_BUDGET; one host read-back (the batch's length) per batch."""
    frames = _device_frames(frames)
    data, offs, at = [], [torch.zeros(1, dtype=torch.int64, device=frames.device)], 0
    for chunk, offsets in _batches(frames, quality):
        data.append(chunk)
        offs.append(offsets[1:] + at)
        at += int(chunk.numel())
    return torch.cat(data), torch.cat(offs)


def jpeg_files(frames, quality: int = 90) -> Iterator[bytes]:
    """the JPEG file of every frame, in order; ONE device-to-host copy of the coded bytes per batch"""
    frames = _device_frames(frames)
    for chunk, offsets in _batches(frames, quality):
        host, o = chunk.cpu().numpy().tobytes(), offsets.cpu().tolist()
        for a, b in zip(o[:-1], o[1:]):
            yield host[a:b]


Encoder = Callable[[object, int], Iterable[bytes]]


def write_jpeg_frames(frames, folder: str, quality: int = 90, encoder: Optional[Encoder] = None) -> str:
    """00000.jpg, 00001.jpg, ... in `folder` (created).  `encoder(frames, quality)` replaces the device encoder (tests)."""
    os.makedirs(folder, exist_ok=True)
    for i, data in enumerate((encoder or jpeg_files)(frames, quality)):
        with open(os.path.join(folder, f"{i:05d}.jpg"), "wb") as fh:
            fh.write(data)
    return folder


# ---- the container -------------------------------------------------------------------------------------------------------------
AVIF_HASINDEX, AVIIF_KEYFRAME = 0x10, 0x10


def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def _jpeg_size(data: bytes) -> Tuple[int, int]:
    """(height, width) from the SOF0 segment of a baseline JPEG file"""
    i = 2
    while i + 4 <= len(data) and data[i] == 0xFF:
        marker, length = data[i + 1], struct.unpack(">H", data[i + 2:i + 4])[0]
        if marker == 0xC0:
            return struct.unpack(">HH", data[i + 5:i + 9])
        if marker == 0xDA:
            break
        i += 2 + length
    raise ValueError("write_mjpeg_avi: a frame is not a baseline JPEG file (no SOF0 segment before the scan)")


def write_mjpeg_avi(frames, path: str, fps: int = 10, quality: int = 90, encoder: Optional[Encoder] = None) -> str:
    """A Motion-JPEG AVI of `frames` (uint8 [F, H, W, 3], device tensor or numpy array): every frame a key frame and a complete JPEG
    file in a word-aligned 00dc chunk, dwScale = 1, dwRate = fps, and an idx1 index whose offsets count from the `movi` fourcc.
    A file that would reach 1 GiB raises ValueError before anything is written (no OpenDML).  `encoder(frames, quality)`, yielding
    one JPEG byte string per frame, replaces the device encoder (tests)."""
    if int(fps) != fps or not 1 <= int(fps) < 1 << 31:
        raise ValueError(f"write_mjpeg_avi: fps must be a positive integer (dwScale is 1), got {fps!r}")
    fps = int(fps)
    files: List[bytes] = []
    total = 12 + (12 + 64 + 12 + 64 + 48) + 12 + 8          # RIFF, hdrl (avih, strl: strh, strf), movi, idx1 -- without frames
    for data in (encoder or jpeg_files)(frames, quality):
        files.append(data)
        total += 8 + len(data) + (len(data) & 1) + 16
        if total >= AVI_LIMIT:
            raise ValueError(f"write_mjpeg_avi: {path} would reach 1 GiB after {len(files)} frames; an AVI without OpenDML "
                             "extensions cannot -- write fewer frames, a lower quality, or a JPEG folder (container='jpg')")
    if not files:
        raise ValueError("write_mjpeg_avi: no frames")
    h, w = _jpeg_size(files[0])
    largest = max(len(d) for d in files)
    index, at = [], 4                                           # offsets count from the `movi` fourcc
    for data in files:
        index.append(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, at, len(data)))
        at += 8 + len(data) + (len(data) & 1)
    avih = struct.pack("<14I", 1000000 // fps, min(largest * fps, 0xFFFFFFFF), 0, AVIF_HASINDEX, len(files), 0, 1, largest, w, h,
                       0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, 1, fps, 0, len(files), largest, 0xFFFFFFFF, 0,
                       0, 0, min(w, 32767), min(h, 32767))   # rcFrame is a RECT of 16-bit values
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
    strl = _chunk(b"LIST", b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf))
    hdrl = _chunk(b"LIST", b"hdrl" + _chunk(b"avih", avih) + strl)
    idx1 = _chunk(b"idx1", b"".join(index))
    assert 12 + len(hdrl) + 8 + at + len(idx1) == total, (len(hdrl), at, len(idx1), total)
    with open(path, "wb") as fh:                                # the frames go to the file as they are: no copy of the movi list
        fh.write(b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", at) + b"movi")
        for data in files:
            fh.write(b"00dc" + struct.pack("<I", len(data)))
            fh.write(data)
            if len(data) & 1:
                fh.write(b"\0")
        fh.write(idx1)
    return path


class AviError(ValueError):
    """read_mjpeg_avi: the file is not what write_mjpeg_avi writes; the message names the field"""


def read_mjpeg_avi(path: str, with_info: bool = False, device=None):
    """The JPEG byte strings of a Motion-JPEG AVI as write_mjpeg_avi lays it out (with_info: and a dict of frames, fps, width,
    height).  device: instead of the byte strings, the frames decoded on that device, uint8 [F, H, W, 3] (video_in.decode_jpeg:
    no Pillow unless a frame's stream is damaged).  Strict: every size and offset has to add up -- RIFF and LIST sizes against the
    file, chunk sizes against their lists, the frame counts of avih and strh against the chunks, idx1 against the chunks' positions
    -- or AviError names it."""
    with open(path, "rb") as fh:
        data = fh.read()

    def need(cond, what):
        if not cond:
            raise AviError(f"{path}: {what}")

    def chunk_at(pos, end, want=None):
        need(pos + 8 <= end, f"chunk header at {pos} runs past {end}")
        fourcc, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        need(want is None or fourcc == want, f"expected {want!r} at {pos}, found {fourcc!r}")
        need(pos + 8 + size <= end, f"{fourcc!r} at {pos}: size {size} runs past {end}")
        return fourcc, pos + 8, size, pos + 8 + size + (size & 1)

    need(len(data) >= 12 and data[:4] == b"RIFF" and data[8:12] == b"AVI ", "not a RIFF AVI file")
    need(struct.unpack("<I", data[4:8])[0] == len(data) - 8, f"RIFF size {struct.unpack('<I', data[4:8])[0]} != file size - 8 = {len(data) - 8}")
    end = len(data)
    _, p, size, after_hdrl = chunk_at(12, end, b"LIST")
    need(data[p:p + 4] == b"hdrl", "the first list is not hdrl")
    hdrl_end = p + size
    _, a, asize, nxt = chunk_at(p + 4, hdrl_end, b"avih")
    need(asize == 56, f"avih size {asize} != 56")
    avih = struct.unpack("<14I", data[a:a + 56])
    _, s, ssize, nxt = chunk_at(nxt, hdrl_end, b"LIST")
    need(data[s:s + 4] == b"strl" and nxt == hdrl_end, "hdrl does not hold exactly avih and one strl")
    strl_end = s + ssize
    _, h_, hsize, nxt = chunk_at(s + 4, strl_end, b"strh")
    need(hsize == 56, f"strh size {hsize} != 56")
    strh = struct.unpack("<4s4sIHHIIIIIIIIhhhh", data[h_:h_ + 56])
    _, f_, fsize, nxt = chunk_at(nxt, strl_end, b"strf")
    need(fsize == 40 and nxt == strl_end, f"strf size {fsize} != 40, or strl holds more than strh and strf")
    strf = struct.unpack("<IiiHH4sIiiII", data[f_:f_ + 40])
    need(strh[0] == b"vids" and strh[1] == b"MJPG" and strf[5] == b"MJPG", f"not an MJPG video stream: {strh[0]!r} {strh[1]!r} {strf[5]!r}")
    need(strf[0] == 40 and strf[3] == 1 and strf[4] == 24, f"strf: biSize {strf[0]}, biPlanes {strf[3]}, biBitCount {strf[4]}")
    need(avih[6] == 1, f"avih.dwStreams {avih[6]} != 1")
    need(strh[6] == 1 and strh[7] >= 1, f"strh: dwScale {strh[6]} != 1 or dwRate {strh[7]} < 1")
    need((avih[8], avih[9]) == (strf[1], strf[2]), f"avih {avih[8]} x {avih[9]} != strf {strf[1]} x {strf[2]}")
    _, m, msize, after_movi = chunk_at(after_hdrl, end, b"LIST")
    need(data[m:m + 4] == b"movi", "the second list is not movi")
    movi_end, pos, frames, where = m + msize, m + 4, [], []
    while pos < movi_end:
        _, d, dsize, nxt = chunk_at(pos, movi_end, b"00dc")
        need(nxt <= movi_end, f"00dc at {pos}: the pad byte runs past movi")
        need(data[d:d + 2] == b"\xff\xd8" and data[d + dsize - 2:d + dsize] == b"\xff\xd9", f"00dc at {pos} is not SOI .. EOI")
        frames.append(data[d:d + dsize])
        where.append((pos - m, dsize))
        pos = nxt
    need(pos == movi_end, f"movi chunks end at {pos}, the list at {movi_end}")
    need(avih[4] == len(frames) == strh[9], f"avih.dwTotalFrames {avih[4]}, strh.dwLength {strh[9]}, {len(frames)} chunks")
    _, x, xsize, after_idx = chunk_at(after_movi, end, b"idx1")
    need(after_idx == end, f"{end - after_idx} bytes after idx1")
    need(xsize == 16 * len(frames), f"idx1 size {xsize} != 16 x {len(frames)}")
    for i, (off, size_) in enumerate(where):
        entry = struct.unpack("<4sIII", data[x + 16 * i:x + 16 * i + 16])
        need(entry == (b"00dc", AVIIF_KEYFRAME, off, size_), f"idx1[{i}] = {entry}, the chunk is at {off} with {size_} bytes")
    if device is not None:
        from . import video_in
        frames = video_in.decode_jpeg(frames, device)
    if with_info:
        return frames, {"frames": len(frames), "fps": strh[7], "width": strf[1], "height": strf[2]}
    return frames
