"""RAFT-large optical flow on libdtk (dtk_raft_* in include/dtk.h): the flow network of preprocessing/extract_trajectories.py.

`RaftLarge(weights, device, operands)` loads a state dict with torchvision's `raft_large` key names, folds the context encoder's
BatchNorms into their convolutions (float64, on the host), packs every convolution for the matrix-core kernel and runs
`dtk_raft_forward`.  `raft_flow_fn` wraps it as the `FlowFn` of flow_trajectories.extract_trajectories with the reference's padding.

PARITY: the key table below and the network it describes are RESTATED FROM MEMORY of torchvision's published raft_large; neither
torchvision nor a trained checkpoint is available where this was written, so the names cannot be verified here and every check
of this module is against tests/raft_ref.py, a plain-torch restatement of the same definition, on seeded weights
(synth.make_raft_weights).  The loader is strict so that a checkpoint whose names differ fails loudly instead of half-loading.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import check, lib

OPERANDS = {"split": _lib.RAFT_SPLIT, "fp16": _lib.RAFT_FP16}
BN_EPS = 1e-5


class ConvSpec(NamedTuple):
    index: int            # position in dtk_raft_model.conv (DTK_RAFT_* in include/dtk.h)
    key: str              # state-dict prefix of the convolution: key + ".weight", key + ".bias"
    cout: int
    cin: int
    kh: int
    kw: int
    stride: int
    pad_h: int
    pad_w: int
    bn: Optional[str]     # prefix of the BatchNorm that follows (context encoder), folded at load time


def _encoder_specs(base: int, prefix: str, batchnorm: bool) -> List[ConvSpec]:
    def cna(i, name, cout, cin, k, stride):   # torchvision's Conv2dNormActivation: .0 the convolution, .1 the norm
        return ConvSpec(i, f"{name}.0", cout, cin, k, k, stride, k // 2, k // 2, f"{name}.1" if batchnorm else None)

    specs = [cna(base, f"{prefix}.convnormrelu", 64, 3, 7, 2)]
    i, cin = base + 1, 64
    for layer, (c, stride) in enumerate(((64, 1), (96, 2), (128, 2)), 1):
        for blk in range(2):
            s = stride if blk == 0 else 1
            p = f"{prefix}.layer{layer}.{blk}"
            specs.append(cna(i, f"{p}.convnormrelu1", c, cin, 3, s))
            specs.append(cna(i + 1, f"{p}.convnormrelu2", c, c, 3, 1))
            i += 2
            if s != 1:
                specs.append(cna(i, f"{p}.downsample", c, cin, 1, s))
                i += 1
            cin = c
    specs.append(ConvSpec(i, f"{prefix}.conv", 256, 128, 1, 1, 1, 0, 0, None))
    return specs


def raft_large_convs() -> List[ConvSpec]:
    """Every convolution of raft_large under its torchvision state-dict name (restated from memory of upstream, see the module
    docstring).  The context encoder's output convolution appears once here (index 31) and is packed as two halves."""
    m, g, u = "update_block.motion_encoder", "update_block.recurrent_block", "update_block.flow_head"
    specs = _encoder_specs(0, "feature_encoder", False) + _encoder_specs(16, "context_encoder", True)
    specs += [ConvSpec(33, f"{m}.convcorr1.0", 256, 324, 1, 1, 1, 0, 0, None),
              ConvSpec(34, f"{m}.convcorr2.0", 192, 256, 3, 3, 1, 1, 1, None),
              ConvSpec(35, f"{m}.convflow1.0", 128, 2, 7, 7, 1, 3, 3, None),
              ConvSpec(36, f"{m}.convflow2.0", 64, 128, 3, 3, 1, 1, 1, None),
              ConvSpec(37, f"{m}.conv.0", 126, 256, 3, 3, 1, 1, 1, None)]
    i = 38
    for gru, (kh, kw) in (("convgru1", (1, 5)), ("convgru2", (5, 1))):
        for gate in ("convz", "convr", "convq"):
            specs.append(ConvSpec(i, f"{g}.{gru}.{gate}", 128, 384, kh, kw, 1, kh // 2, kw // 2, None))
            i += 1
    specs += [ConvSpec(44, f"{u}.conv1", 256, 128, 3, 3, 1, 1, 1, None),
              ConvSpec(45, f"{u}.conv2", 2, 256, 3, 3, 1, 1, 1, None),
              ConvSpec(46, "mask_predictor.convrelu.0", 256, 128, 3, 3, 1, 1, 1, None),
              ConvSpec(47, "mask_predictor.conv", 576, 256, 1, 1, 1, 0, 0, None)]
    return specs


BN_FIELDS = ("weight", "bias", "running_mean", "running_var")


def expected_keys() -> Dict[str, Tuple[int, ...]]:
    """name -> shape of every tensor a raft_large state dict holds (num_batches_tracked: shape ())."""
    keys: Dict[str, Tuple[int, ...]] = {}
    for s in raft_large_convs():
        keys[f"{s.key}.weight"] = (s.cout, s.cin, s.kh, s.kw)
        keys[f"{s.key}.bias"] = (s.cout,)
        if s.bn is not None:
            for f in BN_FIELDS:
                keys[f"{s.bn}.{f}"] = (s.cout,)
            keys[f"{s.bn}.num_batches_tracked"] = ()
    return keys


def check_state_dict(sd: Dict[str, torch.Tensor]) -> None:
    """Strict: a missing key, an unexpected key or a wrong shape raises and names the key."""
    want = expected_keys()
    missing = [k for k in want if k not in sd]
    if missing:
        raise KeyError(f"RAFT weights: missing key {missing[0]!r}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
    extra = [k for k in sd if k not in want]
    if extra:
        raise KeyError(f"RAFT weights: unexpected key {extra[0]!r}" + (f" (and {len(extra) - 1} more)" if len(extra) > 1 else ""))
    for k, shape in want.items():
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"RAFT weights: {k!r} has shape {tuple(sd[k].shape)}, expected {shape}")


def fold_batchnorm(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The state dict in float64 with every eval-mode BatchNorm folded into the convolution before it:
    w' = w g / sqrt(var + eps), b' = (b - mean) g / sqrt(var + eps) + beta.  The BatchNorm keys are dropped."""
    out = {k: v.detach().to("cpu", torch.float64) for k, v in sd.items()}
    for s in raft_large_convs():
        if s.bn is None:
            continue
        g, beta, mean, var = (out.pop(f"{s.bn}.{f}") for f in BN_FIELDS)
        out.pop(f"{s.bn}.num_batches_tracked", None)
        scale = g / torch.sqrt(var + BN_EPS)
        out[f"{s.key}.weight"] = out[f"{s.key}.weight"] * scale.view(-1, 1, 1, 1)
        out[f"{s.key}.bias"] = (out[f"{s.key}.bias"] - mean) * scale + beta
    return out


def weight_scale(w: torch.Tensor) -> float:
    """The power of two that brings max |w| into [2^7, 2^8): the packed lo halves then stay normal fp16 numbers."""
    m = float(w.abs().max())
    if not (m > 0.0 and math.isfinite(m)):
        return 1.0
    return 2.0 ** (7 - math.floor(math.log2(m)))


class PackedConv:
    """One convolution packed for dtk_raft_conv: hi / lo fp16 planes and the fp32 bias on the device."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, stride: int, pad_h: int, pad_w: int, device):
        cout, cin, kh, kw = weight.shape
        w32 = weight.to(device=device, dtype=torch.float32).contiguous()
        n = int(lib().dtk_raft_conv_packed_halves(cout, cin, kh, kw))
        if n == 0:
            raise ValueError(f"unsupported convolution shape {tuple(weight.shape)}")
        self.scale = weight_scale(w32)
        self.hi = torch.empty(n, dtype=torch.float16, device=device)
        self.lo = torch.empty(n, dtype=torch.float16, device=device)
        self.bias = bias.to(device=device, dtype=torch.float32).contiguous()
        check(lib().dtk_raft_conv_pack(w32.data_ptr(), cout, cin, kh, kw, self.scale, self.hi.data_ptr(), self.lo.data_ptr(),
                                       torch.cuda.current_stream(device).cuda_stream))
        self.shape = (cout, cin, kh, kw, stride, pad_h, pad_w)

    def desc(self) -> _lib.RaftConvDesc:
        cout, cin, kh, kw, stride, pad_h, pad_w = self.shape
        return _lib.RaftConvDesc(self.hi.data_ptr(), self.lo.data_ptr(), self.bias.data_ptr(), cin, cout, kh, kw, stride, pad_h, pad_w,
                                 1.0 / self.scale)


def _load(weights) -> Dict[str, torch.Tensor]:
    if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
        weights = torch.load(weights, map_location="cpu")
    if not isinstance(weights, dict):
        raise TypeError("RAFT weights must be a state dict or a path to one")
    return weights


class RaftLarge:
    """RAFT-large inference on the device.  operands: "split" (fp32-grade, the default) or "fp16"."""

    def __init__(self, weights, device="cuda:0", operands: str = "split", max_workspace_bytes: int = 24 << 30):
        if operands not in OPERANDS:
            raise ValueError(f"operands must be one of {sorted(OPERANDS)}, got {operands!r}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("dino_tracker_amd: RaftLarge runs on a GPU -- the hot path has no CPU fallback")
        sd = _load(weights)
        check_state_dict(sd)
        sd = fold_batchnorm(sd)
        self.mode = OPERANDS[operands]
        self.max_workspace_bytes = int(max_workspace_bytes)
        self.convs: List[Optional[PackedConv]] = [None] * _lib.RAFT_NUM_CONVS
        with torch.cuda.device(self.device):
            for s in raft_large_convs():
                w, b = sd[f"{s.key}.weight"], sd[f"{s.key}.bias"]
                if s.key == "context_encoder.conv":      # hidden half (tanh) and context half (ReLU)
                    self.convs[31] = PackedConv(w[:128], b[:128], 1, 0, 0, self.device)
                    self.convs[32] = PackedConv(w[128:], b[128:], 1, 0, 0, self.device)
                    continue
                if s.key == "mask_predictor.conv":       # the mask's 0.25, exact
                    w, b = w * 0.25, b * 0.25
                self.convs[s.index] = PackedConv(w, b, s.stride, s.pad_h, s.pad_w, self.device)
        assert all(c is not None for c in self.convs)
        self.model = _lib.RaftModel()
        for i, c in enumerate(self.convs):
            self.model.conv[i] = c.desc()
        self._ws: Optional[torch.Tensor] = None

    def workspace_bytes(self, n: int, h: int, w: int) -> int:
        return int(lib().dtk_raft_workspace_bytes(n, h, w))

    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    @torch.no_grad()
    def flow(self, src: torch.Tensor, dst: torch.Tensor, num_flow_updates: int = 24) -> torch.Tensor:
        """src, dst [B, 3, H, W] in [-1, 1], H and W divisible by 8 and at least 128 -> the flow src -> dst [B, 2, H, W] fp32 (the last
        of the num_flow_updates predictions).  A batch whose workspace would exceed max_workspace_bytes runs in pieces."""
        if src.dim() != 4 or src.shape[1] != 3 or src.shape != dst.shape:
            raise ValueError(f"src and dst must both be [B, 3, H, W], got {tuple(src.shape)} and {tuple(dst.shape)}")
        B, _, H, W = src.shape
        if H % 8 or W % 8:
            raise ValueError(f"image sizes must be divisible by 8, got {H} x {W}")
        if H // 8 < 16 or W // 8 < 16:
            raise ValueError(f"the 1/8-resolution feature map must be at least 16 x 16: images of at least 128 x 128, got {H} x {W}")
        if num_flow_updates < 1:
            raise ValueError("num_flow_updates must be at least 1")
        src = src.to(device=self.device, dtype=torch.float32).contiguous()
        dst = dst.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty((B, 2, H, W), dtype=torch.float32, device=self.device)
        if B == 0:
            return out
        piece = B
        while piece > 1 and self.workspace_bytes(piece, H, W) > self.max_workspace_bytes:
            piece = (piece + 1) // 2
        with torch.cuda.device(self.device):
            ws = self._workspace(self.workspace_bytes(piece, H, W))
            stream = torch.cuda.current_stream(self.device).cuda_stream
            for i in range(0, B, piece):
                n = min(piece, B - i)
                check(lib().dtk_raft_forward(ctypes.byref(self.model), src[i:i + n].data_ptr(), dst[i:i + n].data_ptr(), n, H, W,
                                             int(num_flow_updates), self.mode, out[i:i + n].data_ptr(), ws.data_ptr(), ws.numel(),
                                             stream))
        return out


def pad_to_8(h: int, w: int) -> List[int]:
    """data_utils.InputPadder ("sintel" mode): [left, right, top, bottom] that bring h x w to multiples of 8."""
    ph, pw = (((h // 8) + 1) * 8 - h) % 8, (((w // 8) + 1) * 8 - w) % 8
    return [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2]


def raft_flow_fn(model: RaftLarge, num_flow_updates: int = 24):
    """A FlowFn for flow_trajectories.extract_trajectories: frames in [0, 1] are replicate-padded to multiples of 8, mapped to
    [-1, 1] (2 x - 1, the weights' transform), and the flow is cropped back -- what torchvision_raft does around its network."""

    @torch.no_grad()
    def flow_fn(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
        h, w = src.shape[-2:]
        pad = pad_to_8(h, w)
        a, b = (torch.nn.functional.pad(x.to(device=model.device, dtype=torch.float32), pad, mode="replicate") * 2.0 - 1.0
                for x in (src, dst))
        flow = model.flow(a, b, num_flow_updates)
        return flow[..., pad[2]:flow.shape[-2] - pad[3], pad[0]:flow.shape[-1] - pad[1]].contiguous()

    return flow_fn


# ---- the stages on their own (tests, timing): thin wrappers of the dtk_raft_* stage entries on NHWC fp32 tensors
def _dev(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("dino_tracker_amd: tensor is not on a GPU -- the hot path has no CPU fallback")
    if t.dtype != torch.float32:
        raise RuntimeError(f"dino_tracker_amd: expected float32, got {t.dtype}")
    return t.data_ptr()


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _slice(t: Optional[torch.Tensor]) -> Tuple[Optional[int], int]:
    """pointer and channel stride of a [..., C] view whose pixels are `stride(-2)` floats apart and whose channels are adjacent"""
    if t is None:
        return None, 0
    if t.stride(-1) != 1:
        raise RuntimeError("dino_tracker_amd: a channel slice must have adjacent channels")
    return _dev(t), int(t.stride(-2))


def conv2d(x: torch.Tensor, conv: PackedConv, out: torch.Tensor, operands: str = "split", act: int = _lib.RAFT_ACT_NONE,
           x2: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, res_relu: bool = False,
           mul: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dtk_raft_conv: x [N, H, W, Cin] (or x | x2 along the channels), written into `out` [N, Ho, Wo, Cout]; all may be channel slices
    (views [..., a:b]) of wider NHWC tensors."""
    N, H, W = x.shape[:3]
    a = _lib.RaftConvArgs()
    a.conv = conv.desc()
    a.N, a.H, a.W, a.mode, a.act, a.res_relu = N, H, W, OPERANDS[operands], act, int(res_relu)
    a.in_split = x.shape[3] if x2 is not None else 0
    (a.in_, a.in_stride), (a.in2, a.in2_stride), (a.out, a.out_stride) = _slice(x), _slice(x2), _slice(out)
    (a.res, a.res_stride), (a.mul, a.mul_stride), (a.gate, a.gate_stride) = _slice(res), _slice(mul), _slice(gate)
    check(lib().dtk_raft_conv(ctypes.byref(a), _stream(x)))
    return out


def instance_norm(x: torch.Tensor, relu: bool = False, res: Optional[torch.Tensor] = None, eps: float = 1e-5) -> torch.Tensor:
    """dtk_raft_instance_norm on a contiguous [N, H, W, C] tensor."""
    N, H, W, C = x.shape
    nb = int(lib().dtk_raft_instance_norm_workspace_bytes(N, H, W, C))
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x)
    check(lib().dtk_raft_instance_norm(_dev(x.contiguous()), _dev(res), _dev(out), N, H, W, C, eps, int(relu), ws.data_ptr(), nb,
                                       _stream(x)))
    return out


def corr_pyramid(f1: torch.Tensor, f2: torch.Tensor, operands: str = "split") -> List[torch.Tensor]:
    """dtk_raft_corr_pyramid: f1, f2 [N, h, w, C] -> the four levels [N, h w, h_l, w_l] (views of one buffer, returned last)."""
    N, h, w, C = f1.shape
    n = int(lib().dtk_raft_pyramid_floats(N, h, w))
    if n == 0:
        raise ValueError(f"the feature map must be at least 16 x 16, got {h} x {w}")
    buf = torch.empty(n, dtype=torch.float32, device=f1.device)
    check(lib().dtk_raft_corr_pyramid(_dev(f1.contiguous()), _dev(f2.contiguous()), N, h, w, C, OPERANDS[operands], _dev(buf),
                                      _stream(f1)))
    levels, off, hl, wl = [], 0, h, w
    for _ in range(4):
        levels.append(buf[off:off + N * h * w * hl * wl].view(N, h * w, hl, wl))
        off += N * h * w * hl * wl
        hl, wl = hl // 2, wl // 2
    return levels + [buf]


def lookup(pyramid: torch.Tensor, flow: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dtk_raft_lookup: pyramid = corr_pyramid(...)[-1]; flow [N, h, w, 2] (a slice is fine) -> [N, h, w, 324]."""
    N, h, w = flow.shape[:3]
    if out is None:
        out = torch.empty((N, h, w, 324), dtype=torch.float32, device=flow.device)
    (fp, fs), (op, os_) = _slice(flow), _slice(out)
    check(lib().dtk_raft_lookup(_dev(pyramid), fp, fs, N, h, w, op, os_, _stream(flow)))
    return out


def upsample(flow: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """dtk_raft_upsample: flow [N, h, w, 2] (a slice is fine), mask [N, h, w, 576] contiguous -> [N, 2, 8 h, 8 w]."""
    N, h, w = flow.shape[:3]
    out = torch.empty((N, 2, 8 * h, 8 * w), dtype=torch.float32, device=flow.device)
    fp, fs = _slice(flow)
    check(lib().dtk_raft_upsample(fp, fs, _dev(mask.contiguous()), N, h, w, _dev(out), _stream(flow)))
    return out
