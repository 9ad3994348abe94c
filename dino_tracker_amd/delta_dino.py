"""Host side of P2: packs a DeltaDINO state dict for the HIP convolution kernels and runs the refinement
(dtk_delta_dino_refine).  Mirrors Tracker.get_refined_embeddings / cache_refined_embeddings (models/tracker.py:113-135)."""
from __future__ import annotations

import ctypes
import os

import torch

from . import ops
from ._lib import Geom, check, lib, make_geom


def weights_key(delta_dino, device):
    """Identity + version of every parameter / BN statistic of the CNN: changes whenever a weight is written."""
    mods = delta_dino.layers
    convs = [mods[0], mods[4], mods[8], mods[12]]
    bns = [mods[1], mods[5], mods[9], mods[13]]
    return tuple((t.data_ptr(), t._version) for m in convs + bns for t in list(m.parameters()) + list(m.buffers())) + (str(device),)


def pack_weights(delta_dino, device):
    """[packed layer 0..3] device tensors; re-packed when any parameter / BN statistic changed."""
    mods = delta_dino.layers
    convs = [mods[0], mods[4], mods[8], mods[12]]
    bns = [mods[1], mods[5], mods[9], mods[13]]
    key = weights_key(delta_dino, device)
    cache = getattr(delta_dino, "_dtk_packed", None)
    if cache is not None and cache[0] == key:
        return cache[1]
    C = delta_dino.channels[-1]
    packed = []
    for l, (cv, bn) in enumerate(zip(convs, bns)):
        n = int(lib().dtk_delta_dino_packed_floats(l, C))
        buf = torch.empty(n, dtype=torch.float32, device=device)
        args = [t.detach().to(device=device, dtype=torch.float32).contiguous()
                for t in (cv.weight, cv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)]
        check(lib().dtk_delta_dino_pack(l, C, *[ops._p(a) for a in args], float(bn.eps), ops._p(buf), ops._stream()))
        packed.append(buf)
    torch.cuda.current_stream().synchronize()  # the temporaries in `args` die here
    delta_dino._dtk_packed = (key, packed)
    return packed


# Operand precision of the 5x5 convolutions of layers 2-4 (include/dtk.h: DTK_DD_SPLIT / DTK_DD_FP16).  A module attribute
# `conv_operands` ("split" / "fp16" / "fp16_v1") on the DeltaDINO instance wins over the environment variable DTK_P2_OPERANDS.
# Default since round 4: plain fp16 operands (fp32 accumulation).  P1 already computes the DINO features with fp16 operands
# (feature error 1.4e-4); the residual CNN's fp16 operands move the refined features by 1e-6 of that on top, and the
# end-to-end error from the video stays where it was (p99 2.7e-4 px, max 3.7e-4 px, flags identical:
# profiles/r04_e2e_error_p2_operands.json) for 20 ms less per 90-frame video.  "split" is the fp32-grade mode (3e-5 of the
# reference's refined features) that the golden-file tests of P2 run.
# "fp16_v1" (DTK_DD_FP16_V1): the values of "fp16", bit for bit, from the kernel sequence it ran before the first layer was fused
# with its blur-pool -- the A / B switch (DTK_P2_OPERANDS=fp16_v1) and the reference of tests/test_gpu_p2_fp16_fused.py.
_OPERAND_MODES = {"split": 0, "fp16": 1, "fp16_v1": 2}
DEFAULT_CONV_OPERANDS = "fp16"


def conv_operand_mode(delta_dino) -> int:
    name = getattr(delta_dino, "conv_operands", None) or os.environ.get("DTK_P2_OPERANDS", DEFAULT_CONV_OPERANDS)
    if name not in _OPERAND_MODES:
        raise ValueError(f"Delta-DINO convolution operands must be one of {sorted(_OPERAND_MODES)}, got {name!r}")
    return _OPERAND_MODES[name]


def _refine(delta_dino, video: torch.Tensor, dino_thwc: torch.Tensor, g: Geom, want_norms: bool = False):
    if delta_dino.training:
        raise RuntimeError("the HIP Delta-DINO path implements eval-mode BatchNorm (inference); call .eval()")
    packed = pack_weights(delta_dino, dino_thwc.device)
    ptrs = (ctypes.c_void_p * 4)(*[p.data_ptr() for p in packed])
    out = torch.empty_like(dino_thwc)
    norms = torch.empty(dino_thwc.shape[:2], dtype=torch.float32, device=dino_thwc.device) if want_norms else None
    ws_bytes = int(lib().dtk_delta_dino_workspace_bytes(g))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dino_thwc.device)
    check(lib().dtk_delta_dino_refine_mode(g, ops._p(video.contiguous(), torch.float32), ops._p(dino_thwc, torch.float32),
                                           ptrs, ops._p(out), ops._p(norms), 0, g.T, conv_operand_mode(delta_dino),
                                           ops._p(ws), ws_bytes, ops._stream()))
    return out, norms


def refine_video_packed(delta_dino, video: torch.Tensor, dino_thwc: torch.Tensor, g: Geom, want_norms: bool = False):
    """All frames; token-major in, token-major out.  want_norms: also the per-cell L2 norms of the refined volume, from the same
    kernel that writes it (align_add sums the squares of the row it has in registers) -> (refined, norms)."""
    out, norms = _refine(delta_dino, video, dino_thwc, g, want_norms=want_norms)
    return (out, norms) if want_norms else out


def refine_packed_subset(delta_dino, frames: torch.Tensor, dino_thwc: torch.Tensor, g: Geom) -> torch.Tensor:
    """A frame subset, token-major in and out: frames [n,3,H,W], dino [n, HW, C] -> refined [n, HW, C]."""
    gg = make_geom(frames.shape[0], g.C, g.video_h, g.video_w, g.patch, g.stride, g.radius)
    return _refine(delta_dino, frames.to(torch.float32), dino_thwc.contiguous(), gg)[0]


def refine_frames(delta_dino, frames: torch.Tensor, dino_chw: torch.Tensor, g: Geom) -> torch.Tensor:
    """Arbitrary frame subset in the reference layout: frames [n,3,H,W], dino [n,C,h,w] -> refined [n,C,h,w]."""
    n = frames.shape[0]
    gg = make_geom(n, g.C, g.video_h, g.video_w, g.patch, g.stride, g.radius)
    thwc, _ = ops.pack_features(dino_chw.to(torch.float32).contiguous())
    out, _ = _refine(delta_dino, frames.to(torch.float32), thwc, gg)
    return ops.unpack_features(out, g.ph, g.pw)


def residual_frames(delta_dino, frames: torch.Tensor, vit_features: torch.Tensor) -> torch.Tensor:
    """DeltaDINO.forward: the aligned CNN output alone (dtk_delta_dino_refine with a zero DINO volume)."""
    n, _, H, W = frames.shape
    _, C, h, w = vit_features.shape
    patch = 14  # align_cnn_vit_features' default, which DeltaDINO.forward does not override (models/utils.py:8)
    g = make_geom(n, C, H, W, patch, delta_dino.vit_stride)
    if (g.ph, g.pw) != (h, w):
        raise NotImplementedError(f"DeltaDINO on the device: ViT grid {h}x{w} must be the patch-14 stride-"
                                  f"{delta_dino.vit_stride} grid of the {H}x{W} frames ({g.ph}x{g.pw})")
    zero = torch.zeros((n, h * w, C), dtype=torch.float32, device=frames.device)
    out, _ = _refine(delta_dino, frames.to(torch.float32), zero, g)
    return ops.unpack_features(out, h, w)
