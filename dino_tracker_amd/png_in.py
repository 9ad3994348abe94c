"""PNG ingest on the device: the files' IDAT payloads go up once, and inflate, the Adler-32 check and the row filters run in libdtk
(csrc/inflate.hip, csrc/inflate_core.h; docs/PNG_DECODE.md).  The format is lossless, so the result equals Pillow's byte for byte.
The host only reads chunk headers:

    parse_png(data)                           (PngHeader, None) for a file the device decodes, else (None, the reason)
    plan_png(datas)                           the headers of several files of one size and colour type
    read_pinned(sources)                      (one pinned buffer of every frame's zlib stream, the plan, the files' bytes)
    decode_png(files_or_bytes, device)        uint8 [T, H, W, C] on the device
    palette_to_l(plte)                        the uint8 [256] table Pillow's convert("L") applies to a palette

Decoded on the device: bit depth 8, colour type 0 (grey, "L"), 2 ("RGB") or 3 (palette, "P": the caller gets the INDICES, or grey
levels through `lut`), not interlaced, no tRNS chunk.  Everything else -- 16-bit and sub-byte depths, colour types 4 and 6,
interlaced files, transparency -- is reported with its reason and stays with the caller's host path.

ONE deliberate difference from Pillow's acceptance: the IDAT chunks' CRCs are not checked (a CRC pass over the compressed bytes on
the host would cost about what the decode does).  What protects the pixels instead is the Adler-32 of the DECODED data, checked on the
device; a frame that fails it -- or any other check of the decoder -- is decoded by Pillow instead.  IHDR's and PLTE's CRCs are
checked here."""
from __future__ import annotations

import io
import os
import struct
import zlib
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

SIGNATURE = b"\x89PNG\r\n\x1a\n"
STREAM_MAX_BYTES = 1 << 28       # dtk_inflate: bit positions are 32-bit
_MODES = {0: "L", 2: "RGB", 3: "P"}
_OTHER_TYPES = {4: "grey with alpha (colour type 4)", 6: "RGBA (colour type 6)"}


@dataclass
class PngHeader:
    height: int
    width: int
    mode: str                        # "L", "RGB" or "P"
    palette: Optional[bytes]         # the PLTE payload of a "P" file
    idat: np.ndarray                 # int64 [K, 2]: byte offset in the file and length of every IDAT payload, in file order

    @property
    def bpp(self) -> int:
        return 3 if self.mode == "RGB" else 1

    @property
    def raw_bytes(self) -> int:      # what the zlib stream holds: a filter byte and a scanline per row
        return self.height * (1 + self.width * self.bpp)


def parse_png(data) -> Tuple[Optional[PngHeader], Optional[str]]:
    """Walk the chunks of one file (bytes, memoryview or uint8 array).  (header, None) when the device decodes it, else (None, why)."""
    buf = bytes(data) if not isinstance(data, np.ndarray) else data.tobytes()
    n = len(buf)
    if buf[:8] != SIGNATURE:
        return None, "no PNG signature"
    if n < 33 or buf[8:16] != b"\x00\x00\x00\rIHDR":
        return None, "the first chunk is not a 13-byte IHDR"
    if struct.unpack(">I", buf[29:33])[0] != zlib.crc32(buf[12:29]):
        return None, "IHDR: CRC mismatch"
    width, height, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", buf[16:29])
    if ctype in _OTHER_TYPES:
        return None, _OTHER_TYPES[ctype]
    if ctype not in _MODES:
        return None, f"colour type {ctype}"
    if depth != 8:
        return None, f"bit depth {depth}"
    if lace != 0:
        return None, "interlaced (Adam7)"
    if comp != 0 or flt != 0:
        return None, "compression or filter method other than 0"
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        return None, f"{height} x {width}: a side of 0 or above 65535"
    palette, idat, at, ended, closed = None, [], 33, False, False
    while at < n:
        if at + 12 > n:
            return None, f"chunk header at byte {at} runs past the file"
        length, kind = struct.unpack(">I4s", buf[at:at + 8])
        if at + 12 + length > n:
            return None, f"chunk {kind!r} at byte {at} runs past the file"
        if kind == b"IDAT":
            if closed:
                return None, "IDAT chunks are not consecutive"
            idat.append((at + 8, length))
        elif idat:
            closed = True
        if kind == b"PLTE":
            if idat or palette is not None:
                return None, "PLTE after IDAT, or twice"
            if length % 3 or not 3 <= length <= 768:
                return None, "PLTE: not 1 .. 256 entries of three bytes"
            if struct.unpack(">I", buf[at + 8 + length:at + 12 + length])[0] != zlib.crc32(buf[at + 4:at + 8 + length]):
                return None, "PLTE: CRC mismatch"
            palette = buf[at + 8:at + 8 + length]
        elif kind == b"tRNS":
            return None, "transparency (tRNS chunk)"
        elif kind == b"IEND":
            ended = True
            break
        at += 12 + length
    if not ended:
        return None, "no IEND chunk"
    if not idat:
        return None, "no IDAT chunk"
    if ctype == 3 and palette is None:
        return None, "palette image without PLTE"
    idat_arr = np.asarray(idat, dtype=np.int64).reshape(-1, 2)
    if int(idat_arr[:, 1].sum()) > STREAM_MAX_BYTES:
        return None, "IDAT data longer than 256 MiB"
    return PngHeader(height, width, _MODES[ctype], palette if ctype == 3 else None, idat_arr), None


def palette_to_l(plte: bytes) -> np.ndarray:
    """uint8 [256]: what Pillow's convert("L") makes of a palette entry, L = (19595 R + 38470 G + 7471 B + 32768) >> 16; zero beyond
    the palette's entries."""
    p = np.frombuffer(plte, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
    lut = np.zeros(256, dtype=np.uint8)
    lut[:p.shape[0]] = (19595 * p[:, 0] + 38470 * p[:, 1] + 7471 * p[:, 2] + 32768) >> 16
    return lut


@dataclass
class PngPlan:
    """what dtk_inflate / dtk_adler32 / dtk_png_unfilter take for F files of one size and colour type"""
    frames: int
    height: int
    width: int
    mode: str
    headers: List[PngHeader]
    streams: np.ndarray     # int64 [F, 4]: byte offset in the joined stream buffer, byte length, byte offset in the raw buffer, raw bytes

    @property
    def bpp(self) -> int:
        return 3 if self.mode == "RGB" else 1


def plan_png(datas: Sequence) -> Tuple[Optional[PngPlan], Optional[str]]:
    """Parse every file; (plan, None) when all are eligible and of one size and colour type, else (None, "<index>: <reason>").  The
    plan's stream f is the file's IDAT payloads one after the other, the streams one after the other."""
    if not len(datas):
        return None, "no files"
    headers: List[PngHeader] = []
    for f, data in enumerate(datas):
        h, why = parse_png(data)
        if h is None:
            return None, f"file {f}: {why}"
        if headers and (h.height, h.width, h.mode) != (headers[0].height, headers[0].width, headers[0].mode):
            first = headers[0]
            return None, f"file {f}: {h.height} x {h.width} {h.mode}, file 0 is {first.height} x {first.width} {first.mode}"
        headers.append(h)
    sizes = np.asarray([int(h.idat[:, 1].sum()) for h in headers], dtype=np.int64)
    streams = np.empty((len(headers), 4), dtype=np.int64)
    streams[:, 0] = np.concatenate(([0], np.cumsum(sizes)))[:-1]
    streams[:, 1] = sizes
    streams[:, 2] = np.arange(len(headers), dtype=np.int64) * headers[0].raw_bytes
    streams[:, 3] = headers[0].raw_bytes
    return PngPlan(len(headers), headers[0].height, headers[0].width, headers[0].mode, headers, streams), None


# ---- bytes: one pinned buffer of zlib streams, one upload ----------------------------------------------------------------------------
Source = Union[str, os.PathLike, bytes, bytearray, memoryview]


def _read(source: Source) -> bytes:
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    with open(source, "rb") as fh:
        return fh.read()


def read_pinned(sources: Sequence[Source]) -> Tuple[Optional[torch.Tensor], Optional[PngPlan], List[bytes], Optional[str]]:
    """(pinned uint8 buffer with every frame's IDAT payloads, chunk framing stripped: one contiguous zlib stream per frame --, the
    plan, the files' bytes, None), or (None, None, the files' bytes, why) when the files do not plan."""
    datas = [_read(s) for s in sources]
    plan, why = plan_png(datas)
    if plan is None:
        return None, None, datas, why
    pinned = torch.empty(max(1, int(plan.streams[:, 1].sum())), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    whole = pinned.numpy()
    for data, h, s in zip(datas, plan.headers, plan.streams):
        at = int(s[0])
        view = np.frombuffer(data, dtype=np.uint8)
        for off, length in h.idat.tolist():
            whole[at:at + length] = view[off:off + length]
            at += length
    return pinned, plan, datas, None


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("dino_tracker_amd: the PNG decoder needs a GPU device -- the hot path has no CPU fallback")
    return device


def _pillow(data: bytes, mode: str) -> np.ndarray:
    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:
        img.load()
        frame = np.asarray(img if img.mode == mode else img.convert(mode))
    return np.ascontiguousarray(frame)


def decode_planned(pinned: torch.Tensor, plan: PngPlan, datas: List[bytes], device, palette: str = "index", fallback: bool = True,
                   with_status: bool = False):
    """dtk_inflate -> dtk_adler32 -> dtk_png_unfilter: uint8 [T, H, W, C] on `device` (C = 3 for RGB, else 1).  A "P" plan yields
    the palette indices (palette="index") or Pillow's convert("L") of them (palette="L", through a per-frame table).  After the
    launches ONE host read, the frames' status; a frame whose status is not zero is decoded by Pillow instead and uploaded into its
    slot (`fallback`), which raises what Pillow raises."""
    from . import ops
    if palette not in ("index", "L"):
        raise ValueError(f"decode_planned: palette must be 'index' or 'L', got {palette!r}")
    device = _device(device)
    stream = pinned.to(device, non_blocking=True)
    raw, status = ops.inflate(stream, plan.streams, int(plan.frames * plan.headers[0].raw_bytes), wrapper=True)
    ops.adler32(stream, plan.streams, raw, status)
    lut = None
    if plan.mode == "P" and palette == "L":
        lut = torch.from_numpy(np.stack([palette_to_l(h.palette) for h in plan.headers])).to(device)
    out = ops.png_unfilter(raw, plan.frames, plan.height, plan.width, plan.bpp, status, lut)
    host_status = status.cpu()                       # the one host read
    if fallback and bool(host_status.any()):
        mode = "L" if (plan.mode == "P" and palette == "L") else plan.mode
        for f in torch.nonzero(host_status).flatten().tolist():
            frame = _pillow(datas[f], mode).reshape(plan.height, plan.width, plan.bpp)
            out[f] = torch.from_numpy(frame).to(device)
    return (out, host_status) if with_status else out


def decode_png(sources: Sequence[Source], device="cuda:0", palette: str = "index", fallback: bool = True, with_status: bool = False):
    """uint8 [T, H, W, C] on `device` from PNG files (paths) or byte strings of one size and colour type.  ValueError with the
    reason when a file is not of the kind the device decodes (module docstring).  with_status: also the int32 [T] status as the
    device reported it (host tensor; ops.INFLATE_S_* and ops.PNG_S_FILTER bits)."""
    pinned, plan, datas, why = read_pinned(sources)
    if plan is None:
        raise ValueError(f"decode_png: not decodable on the device -- {why}")
    return decode_planned(pinned, plan, datas, device, palette, fallback, with_status)
