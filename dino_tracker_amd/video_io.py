"""Video ingest on the device: frames are decoded -- baseline 4:2:0 JPEG folders by libdtk (video_in.py, csrc/jpeg_decode.hip:
the compressed bytes go up; 4:4:4, 4:2:2 and gray ones, and progressive files of all four layouts, when DTK_JPEG_DECODE=device asks for it), 8-bit grey or RGB PNG folders by libdtk as well when DTK_PNG_DECODE selects it (png_in.py,
csrc/inflate.hip), everything else by Pillow on the host and uploaded once as uint8 -- and LANCZOS-resized by libdtk
(csrc/resize.hip) with Pillow's own 8-bit arithmetic, so the result is bit-equal to `Image.resize(..., Image.LANCZOS)` followed by
`ToTensor` -- what data/data_utils.py:79-104 (`load_video`) and :47-52 (`resize_tensor_frames_lanczos`) compute on the CPU.

Pillow's resampler (src/libImaging/Resample.c) is two separable passes of integer arithmetic on uint8 with a uint8 intermediate,
horizontal first.  The filter itself is evaluated HERE, on the host, in Python floats (C doubles, libm's sin, as Pillow does) into
22-bit fixed-point tables; the kernels only multiply and add, so they are exact whatever the device's float unit does."""
from __future__ import annotations

import functools
import math
import os
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops

PRECISION_BITS = 22   # Resample.c: 32 - 8 - 2
LANCZOS_SUPPORT = 3.0


def _lanczos(x: float) -> float:
    """Resample.c lanczos_filter / sinc_filter."""
    if not -3.0 <= x < 3.0:
        return 0.0

    def sinc(v: float) -> float:
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    return sinc(x) * sinc(x / 3)


@functools.lru_cache(maxsize=64)
def lanczos_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc for the whole axis (box = (0, in_size)): int32 weights [out, ksize]
    (zero beyond a row's count) and int32 bounds [out, 2] = (first input index, count).  Read-only arrays, cached per size pair."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"lanczos_tables: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = LANCZOS_SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    k = np.zeros((out_size, ksize), dtype=np.int64)
    b = np.zeros((out_size, 2), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ws = [_lanczos((j + xmin - center + 0.5) * ss) for j in range(xmax)]
        ww = 0.0
        for v in ws:
            ww += v
        if ww != 0.0:
            ws = [v / ww for v in ws]
        k[i, :xmax] = [int(v * one - 0.5) if v < 0 else int(v * one + 0.5) for v in ws]
        b[i] = (xmin, xmax)
    # what the kernels rely on: 24-bit multiplies are exact, and no row can overflow the int32 accumulator
    assert int(np.abs(k).max()) < (1 << 23), (in_size, out_size)
    assert int(255 * np.abs(k).sum(axis=1).max()) + (1 << 21) < (1 << 31), (in_size, out_size)
    k = k.astype(np.int32)
    k.setflags(write=False)
    b.setflags(write=False)
    return k, b


_DEVICE_TABLES: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}
_DEVICE_LUT: Dict[torch.device, torch.Tensor] = {}


def _device_tables(in_size: int, out_size: int, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    key = (in_size, out_size, device)
    if key not in _DEVICE_TABLES:
        k, b = lanczos_tables(in_size, out_size)
        _DEVICE_TABLES[key] = (torch.from_numpy(k.copy()).to(device), torch.from_numpy(b.copy()).to(device))
    return _DEVICE_TABLES[key]


def _u8_to_f32(device: torch.device) -> torch.Tensor:
    """ToTensor's u8 / 255 for every byte, rounded by the HOST: the fp32 output is a table look-up."""
    if device not in _DEVICE_LUT:
        _DEVICE_LUT[device] = torch.arange(256, dtype=torch.uint8).float().div(255).to(device)
    return _DEVICE_LUT[device]


def resize_lanczos(frames_u8: torch.Tensor, h: int, w: int, out: str = "u8", force_general: bool = False) -> torch.Tensor:
    """Image.resize((w, h), Image.LANCZOS) of device uint8 frames [N, H, W, C] or [H, W, C] (C = 1 or 3).
    out="u8": uint8 [N, h, w, C];  out="f32": float32 [N, C, h, w] = ToTensor (u8 / 255).  `force_general` takes the two-launch
    form of the kernel where the fused one would run (tests)."""
    if out not in ("u8", "f32"):
        raise ValueError(f"resize_lanczos: out must be 'u8' or 'f32', got {out!r}")
    if not frames_u8.is_cuda:
        raise RuntimeError("dino_tracker_amd: tensor is not on a GPU -- the hot path has no CPU fallback")
    single = frames_u8.dim() == 3
    x = frames_u8[None] if single else frames_u8
    if x.dim() != 4 or x.dtype != torch.uint8 or x.shape[-1] not in (1, 3) or x.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: frames must be [N, H, W, C] or [H, W, C] uint8 with C in (1, 3), got "
                           f"{tuple(frames_u8.shape)} {frames_u8.dtype}")
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"resize_lanczos: the output size must be positive, got {h} x {w}")
    H, W = int(x.shape[1]), int(x.shape[2])
    dev = x.device
    kx, bx = _device_tables(W, w, dev) if W != w else (None, None)
    ky, by = _device_tables(H, h, dev) if H != h else (None, None)
    y = ops.resize_u8(x.contiguous(), h, w, kx, bx, ky, by, _u8_to_f32(dev) if out == "f32" else None,
                      ops.RESIZE_OUT_F32_CHW if out == "f32" else ops.RESIZE_OUT_U8_HWC,
                      ops.RESIZE_FORCE_GENERAL if force_general else 0)
    return y[0] if single else y


def resize_tensor_frames_lanczos(frames: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """data/data_utils.py:47-52 on the device: float frames [T, C, H, W] -> ToPILImage (mul(255) in fp32, truncated to uint8 --
    so v / 255 * 255 may land one below v, as there) -> LANCZOS resize -> ToTensor.  The quantisation and the change of layout
    are torch on the device; the resize is libdtk's."""
    if not frames.is_cuda:
        raise RuntimeError("dino_tracker_amd: tensor is not on a GPU -- the hot path has no CPU fallback")
    if frames.dim() != 4 or not frames.is_floating_point() or frames.shape[1] not in (1, 3):
        raise RuntimeError(f"dino_tracker_amd: frames must be float [T, C, H, W] with C in (1, 3), got {tuple(frames.shape)} "
                           f"{frames.dtype}")
    u8 = frames.float().mul(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return resize_lanczos(u8, h, w, out="f32")


def video_files(video_folder) -> list:
    """data/data_utils.py:91-92: *.jpg then *.png, sorted together."""
    path = Path(video_folder)
    return sorted(list(path.glob("*.jpg")) + list(path.glob("*.png")))


def _decode_pinned(files) -> Optional[torch.Tensor]:
    """All frames into ONE pinned uint8 [T, H, W, C] buffer; None when they are not all RGB or all L of one size."""
    from PIL import Image
    buf = view = None
    first = None
    for t, f in enumerate(files):
        with Image.open(str(f)) as img:
            if img.mode not in ("RGB", "L") or (first is not None and (img.mode, img.size) != first):
                return None
            if first is None:
                first = (img.mode, img.size)
                buf = torch.empty((len(files), img.size[1], img.size[0], len(img.mode)), dtype=torch.uint8, pin_memory=True)
                view = buf.numpy()
            view[t] = np.asarray(img).reshape(view.shape[1:])
    return buf


# The samplings (video_in.S420, S422, S444, GRAY = 0 .. 3) DTK_JPEG_DECODE=auto decodes on the device.  The bar is the one of
# PNG_AUTO_USES_DEVICE below: not slower than the host path beyond the host path's own spread at every measured point
# (docs/MEASUREMENTS.md "JPEG decode" for 4:2:0, "JPEG decode: other samplings" for the rest).
JPEG_AUTO_SAMPLINGS = (0,)


def _decode_jpeg_device(files, device: torch.device) -> Optional[torch.Tensor]:
    """uint8 [T, H, W, 3] (gray files: [T, H, W, 1]) on the device when every file is a JPEG the device decodes
    (video_in.parse_jpeg_sampled) and all are of one size and one sampling, else None: the routing is decided from the headers, before
    anything is uploaded.  DTK_JPEG_DECODE = host | device | auto (the default): `host` keeps Pillow for everything; `device` takes
    the device decoder for every eligible folder -- a folder of PROGRESSIVE files that video_in.plan_jpeg_progressive accepts
    included --; `auto` for the eligible baseline folders whose sampling is in JPEG_AUTO_SAMPLINGS.  Which entropy stage a baseline
    folder that goes to the device runs is DTK_JPEG_ENTROPY's business (video_in.entropy_mode): `sequential`, the default, or
    `parallel` -- for files without restart markers; the frames are the same."""
    mode = os.environ.get("DTK_JPEG_DECODE", "auto")
    if mode not in ("auto", "device", "host"):
        raise ValueError(f"DTK_JPEG_DECODE must be auto, device or host, got {mode!r}")
    if mode == "host" or any(Path(f).suffix != ".jpg" for f in files):
        return None
    from . import video_in
    pinned, views = video_in.read_pinned(files)
    plan, _ = video_in.plan_jpeg_sampled(views)
    if plan is None and mode == "device":
        # a folder of progressive files (video_in.parse_jpeg_progressive): opt-in only, whatever JPEG_AUTO_SAMPLINGS says
        # (docs/MEASUREMENTS.md "JPEG decode: progressive")
        progressive, _ = video_in.plan_jpeg_progressive(views)
        return None if progressive is None else video_in.decode_planned_progressive(pinned, views, progressive, device)
    if plan is None or (mode == "auto" and plan.sampling not in JPEG_AUTO_SAMPLINGS):
        return None
    return video_in.decode_planned(pinned, views, plan, device)


# What DTK_PNG_DECODE=auto selects.  The project's bar for ingest: the device path only where it is not slower than the host path beyond
# the host path's own spread, at every size and compression level measured (docs/MEASUREMENTS.md "PNG decode").
PNG_AUTO_USES_DEVICE = False


def decode_png_device(files, device: torch.device, modes=("RGB", "L"), palette: str = "index") -> Optional[torch.Tensor]:
    """uint8 [T, H, W, C] on the device when every file is a PNG the device decodes (png_in.parse_png), all are of one size and of
    one colour type among `modes`, else None: the routing is decided from the chunk headers, before anything is uploaded.
    DTK_PNG_DECODE = host | device | auto (the default): `host` keeps Pillow for everything, `device` takes the device decoder for
    every eligible folder, `auto` does what PNG_AUTO_USES_DEVICE says."""
    mode = os.environ.get("DTK_PNG_DECODE", "auto")
    if mode not in ("auto", "device", "host"):
        raise ValueError(f"DTK_PNG_DECODE must be auto, device or host, got {mode!r}")
    if mode == "host" or (mode == "auto" and not PNG_AUTO_USES_DEVICE) or not files or any(Path(f).suffix != ".png" for f in files):
        return None
    from . import png_in
    pinned, plan, datas, _ = png_in.read_pinned(files)
    if plan is None or plan.mode not in modes:
        return None
    return png_in.decode_planned(pinned, plan, datas, device, palette=palette)


def load_video(video_folder, resize=None, num_frames: Optional[int] = None, device="cuda:0") -> torch.Tensor:
    """data/data_utils.py:79-104 with the resize on the device: the frames of `video_folder` in file order (the first
    `num_frames`) as uint8 on the device, LANCZOS-resized to `resize` = (h, w) and converted as ToTensor does -> float32
    [T, C, h, w] on `device`, bit-equal to the host path.  A folder of baseline 4:2:0 JPEG files of one size is decoded on the device
    from its compressed bytes (a frame whose stream is damaged is decoded by Pillow instead) -- with DTK_JPEG_DECODE=device a folder
    of 4:4:4, 4:2:2 or gray ones, or of progressive files, as well (_decode_jpeg_device) --, and so is a folder of 8-bit grey or RGB
    PNG files of one size when DTK_PNG_DECODE selects the device (decode_png_device; palette, 16-bit, alpha and interlaced files and
    mixed .jpg / .png folders never do); other frames are decoded by Pillow on the host and uploaded once.  Frames that are not all RGB or all L of one size take the host path (train.load_video) and are
    uploaded afterwards."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("dino_tracker_amd: video_io.load_video needs a GPU device -- the hot path has no CPU fallback")
    files = video_files(video_folder)
    files = files[:num_frames] if num_frames is not None else files
    if not files:
        raise RuntimeError(f"dino_tracker_amd: no *.jpg / *.png frames in {video_folder}")
    frames = _decode_jpeg_device(files, device)
    if frames is None:
        frames = decode_png_device(files, device)
    if frames is not None:
        h, w = (int(resize[0]), int(resize[1])) if resize is not None else (int(frames.shape[1]), int(frames.shape[2]))
        return resize_lanczos(frames, h, w, out="f32")
    frames = _decode_pinned(files)
    if frames is None:
        from .train import load_video as host_load_video
        video = host_load_video(video_folder, resize=resize)
        return (video[:num_frames] if num_frames is not None else video).to(device)
    frames = frames.to(device, non_blocking=True)
    h, w = (int(resize[0]), int(resize[1])) if resize is not None else (int(frames.shape[1]), int(frames.shape[2]))
    return resize_lanczos(frames, h, w, out="f32")
