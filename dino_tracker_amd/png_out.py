"""PNG output on the device: frames leave it as complete PNG files (csrc/deflate.hip, docs/PNG_ENCODE.md) -- the row filters, DEFLATE,
the Adler-32, the CRC-32 and the chunk framing all run in libdtk; the host builds the 33 bytes that do not depend on the pixels.

    png_header(h, w, channels)                the signature and the IHDR chunk with its CRC
    encode_png(frames, filter)                device uint8 [F, H, W, 1 or 3] (or [F, H, W]) -> (device uint8 [bytes], int64 [F + 1] offsets)
    png_files(frames, filter)                 the files as byte strings; ONE device-to-host copy of the coded bytes per batch
    write_png_frames(frames, folder)          00000.png ..., the names load_video, load_masks and the reference's loaders glob
    deflate(datas, device, wrapper)           zlib (or raw DEFLATE) streams of byte strings, through the same kernels (tests, tools)

Written: 8-bit, non-interlaced, colour type 0 (grey, one channel) or 2 (RGB) -- exactly what png_in.parse_png accepts, so what is
written here is read back on the device too.  The format is lossless: a decoder returns the frames to the bit.  The filter stage, the
Adler-32 and the CRC-32 are defined to the bit; the DEFLATE bytes are valid and deterministic but not zlib's (docs/PARITY.md).  There
is no CPU encoder here -- CPU tensors are refused, numpy arrays are uploaded."""
from __future__ import annotations

import os
import struct
import zlib
from typing import Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

SIGNATURE = b"\x89PNG\r\n\x1a\n"
WORKSPACE_BUDGET = 256 << 20         # device bytes of one batch's workspace (about six times the frames, docs/PNG_ENCODE.md section 6)
WORST_CASE_LIMIT = 64 << 20          # output buffers up to this size are allocated at the worst-case bound: no retry can happen
GUESS_RATIO = 0.6                    # beyond it: this share of the raw bytes, and one retry when it is short
FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}


# ---- host: the header ------------------------------------------------------------------------------------------------------------
def png_header(h: int, w: int, channels: int) -> bytes:
    """The 33 bytes in front of the IDAT chunk: signature, then IHDR (width, height, bit depth 8, colour type 0 for one channel and 2
    for three, compression 0, filter method 0, not interlaced) with its length and CRC."""
    h, w, channels = int(h), int(w), int(channels)
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"png_header: a frame must be 1 .. 65535 pixels each way, got {h} x {w}")
    if channels not in (1, 3):
        raise ValueError(f"png_header: 1 (grey) or 3 (RGB) channels, got {channels}")
    body = b"IHDR" + struct.pack(">IIBBBBB", w, h, 8, 0 if channels == 1 else 2, 0, 0, 0)
    return SIGNATURE + struct.pack(">I", 13) + body + struct.pack(">I", zlib.crc32(body))


def _filter_code(filter) -> int:
    code = FILTERS.get(filter, filter) if isinstance(filter, str) else filter
    if not isinstance(code, (int, np.integer)) or isinstance(code, bool) or not 0 <= int(code) <= 5:
        raise ValueError(f"filter must be one of {sorted(FILTERS)} or 0 .. 5, got {filter!r}")
    return int(code)


# ---- device: frames -> PNG files ---------------------------------------------------------------------------------------------------
def _device_frames(frames) -> torch.Tensor:
    if isinstance(frames, torch.Tensor):
        if not frames.is_cuda:
            raise RuntimeError("dino_tracker_amd: tensor is not on a GPU -- the hot path has no CPU fallback")
        t = frames
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(frames))).to("cuda:0")
    if t.dim() == 3:
        t = t.unsqueeze(-1)
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] not in (1, 3) or t.numel() == 0:
        raise TypeError(f"frames must be uint8 [F, H, W], [F, H, W, 1] or [F, H, W, 3] with F, H, W >= 1, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def frames_per_batch(F: int, H: int, W: int, channels: int, budget: Optional[int] = None) -> int:
    """frames of one dtk_png_encode call: as many as keep its workspace inside `budget` (WORKSPACE_BUDGET) bytes, at least one"""
    from . import ops
    budget = WORKSPACE_BUDGET if budget is None else int(budget)
    return max(1, min(int(F), budget // max(1, ops.png_encode_workspace_bytes(1, H, W, channels))))


def first_capacity(F: int, H: int, W: int, channels: int) -> int:
    """The capacity policy of video_out.first_capacity: the worst-case bound where that is small, else the framing and GUESS_RATIO of
    the raw bytes per frame -- the call reports the needed size when that is short, and ops.png_encode retries once."""
    from . import ops
    worst = ops.png_worst_case_bytes(F, H, W, channels)
    if worst <= WORST_CASE_LIMIT:
        return worst
    return min(worst, F * (ops.PNG_FILE_OVERHEAD + int(GUESS_RATIO * H * (1 + W * channels)) + 4096))


def _batches(frames: torch.Tensor, filter: int) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
    from . import ops
    F, H, W, C = (int(v) for v in frames.shape)
    header = torch.frombuffer(bytearray(png_header(H, W, C)), dtype=torch.uint8).to(frames.device)
    step = frames_per_batch(F, H, W, C)
    for f0 in range(0, F, step):
        part = frames[f0:f0 + step]
        yield ops.png_encode(part, header, filter, first_capacity(int(part.shape[0]), H, W, C))


def encode_png(frames, filter="adaptive") -> Tuple[torch.Tensor, torch.Tensor]:
    """frames uint8 [F, H, W, 1 or 3] (or [F, H, W]) on the device -> (uint8 [bytes], int64 [F + 1]), both on the device: file f is
    bytes[offsets[f] : offsets[f + 1]], a complete PNG file.  filter: "adaptive" (per row, the PNG specification's heuristic), or one
    of "none", "sub", "up", "average", "paeth" for every row.  Frames are encoded in batches sized to WORKSPACE_BUDGET; one host
    read-back (the batch's length) per batch."""
    code = _filter_code(filter)
    frames = _device_frames(frames)
    data, offs, at = [], [torch.zeros(1, dtype=torch.int64, device=frames.device)], 0
    for chunk, offsets in _batches(frames, code):
        data.append(chunk)
        offs.append(offsets[1:] + at)
        at += int(chunk.numel())
    return torch.cat(data), torch.cat(offs)


def png_files(frames, filter="adaptive") -> Iterator[bytes]:
    """the PNG file of every frame, in order; ONE device-to-host copy of the coded bytes per batch"""
    code = _filter_code(filter)
    frames = _device_frames(frames)
    for chunk, offsets in _batches(frames, code):
        host, o = chunk.cpu().numpy().tobytes(), offsets.cpu().tolist()
        for a, b in zip(o[:-1], o[1:]):
            yield host[a:b]


def write_png_frames(frames, folder: str, filter="adaptive") -> str:
    """00000.png, 00001.png, ... in `folder` (created)"""
    os.makedirs(folder, exist_ok=True)
    for i, data in enumerate(png_files(frames, filter)):
        with open(os.path.join(folder, f"{i:05d}.png"), "wb") as fh:
            fh.write(data)
    return folder


def deflate(datas: Sequence[Union[bytes, bytearray, memoryview]], device="cuda:0", wrapper: bool = True) -> List[bytes]:
    """The zlib (wrapper) or raw DEFLATE stream of every byte string, compressed on `device` in one call: one upload, one download."""
    from . import ops
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("dino_tracker_amd: the DEFLATE encoder needs a GPU device -- the hot path has no CPU fallback")
    if not len(datas):
        return []
    sizes = np.asarray([len(d) for d in datas], dtype=np.int64)
    ranges = np.stack([np.concatenate(([0], np.cumsum(sizes)))[:-1], sizes], axis=1)
    blob = b"".join(bytes(d) for d in datas) or b"\x00"
    data = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(device)
    out, offsets = ops.deflate(data, ranges, wrapper)
    host, o = out.cpu().numpy().tobytes(), offsets.cpu().tolist()
    return [host[a:b] for a, b in zip(o[:-1], o[1:])]
