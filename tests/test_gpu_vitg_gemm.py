"""-m gpu: the GEMM stages of ViT-g/14 (D = 1536) ALONE, through dtk_vit_gemm / dtk_vit_gemm_split, against float64 on the operands
the device read (tests/vitg_ref.py, tests/vit_gemm_ref.py; the CPU counterpart tests/test_vitg_reference.py shows that the checks
reject wrong kernels).

  FC1_SWIGLU   the packed w12 GEMM with the SwiGLU epilogue: the realistic classes, per-element bound of vitg_ref.bound_fc1
  FC2_SWIGLU   w3 (N = 1536, K = 4096), QKV (N = 4608) and PROJ at D = 1536: the exact class bit for bit, the realistic one bounded
on the four kernel forms of launch_gemm / launch_gemm_split at this width --
  wide         flags 0            gemm_wide_kernel<T, EPI, true>        row tile 256
  tiled        TILED_GEMMS        gemm_tiled_kernel<T, EPI>             row tile 128
  split_dma    0, split planes    gemm_split_dma_kernel<T, SEPI, true>  row tile 256
  split_tiled  TILED_GEMMS, split gemm_split_kernel<T, SEPI>            row tile 128
Every output has a guard band behind its last row that must come back untouched.  Each case prints its largest |got - ref| / bound;
the record of those figures is docs/PARITY.md ("ViT-g/14")."""
import ctypes

import pytest
import torch

import vit_gemm_ref as R
import vitg_ref as G
from dino_tracker_amd import _lib, ops
from dino_tracker_amd._lib import check, lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A
TILED, WS_V1, WIDE_V1 = _lib.VIT_TILED_GEMMS, _lib.VIT_GEMM_WS_V1, _lib.VIT_GEMM_WIDE_V1
assert (G.FC1_SWIGLU, G.FC2_SWIGLU) == (_lib.VIT_GEMM_FC1_SWIGLU, _lib.VIT_GEMM_FC2_SWIGLU)
D = G.D_G

PATHS = {"wide": (0, False, 256), "tiled": (TILED, False, 128), "split_dma": (0, True, 256), "split_tiled": (TILED, True, 128)}


def rows_of(t):
    return [1, t - 1, t, t + 1, 3 * t + 17]


class Guarded:
    """A tensor followed by a guard band; both start as a sentinel bit pattern (`zero`: the tensor as zeros -- Q / K / V^T padding)."""

    def __init__(self, shape, dtype, guard, zero=False, init=None):
        n = 1
        for s in shape:
            n *= s
        self.n, self.bits = n, (torch.int32 if dtype == torch.float32 else torch.int16)
        self.sent = SENT32 if dtype == torch.float32 else SENT16
        self.flat = torch.full((n + guard,), self.sent, dtype=self.bits, device=DEV)
        self.t = self.flat[:n].view(dtype).view(shape)
        if zero:
            self.t.zero_()
        if init is not None:
            self.t.copy_(init)

    def guard_ok(self):
        return bool((self.flat[self.n:] == self.sent).all())


def run_stage(o, flags, ovf=None, D_arg=D, role_arg=None):
    """One launch of the stage on the operands `o`; returns the outputs in the stage's layouts.  FC1_SWIGLU: `o` holds w12 / b12 in
    upstream row order, the device is given the packed rows (vitg_ref.pack_rows)."""
    role = o.get("role_dev", o["role"]) if role_arg is None else role_arg
    dtype, split, rows = o["dtype"], o["split"], o["rows"]
    swiglu = o["role"] == G.FC1_SWIGLU
    W, W_lo, bias = o["W"], o.get("W_lo"), o["bias"]
    if swiglu:
        W, bias = G.pack_rows(W), G.pack_rows(bias)
        W_lo = G.pack_rows(W_lo) if split else None
    N = W.shape[0] // 2 if swiglu else W.shape[0]
    a = _lib.VitGemmArgs()
    a.role, a.D, a.flags, a.operand_type, a.rows = role, D_arg, flags, (_lib.OPERAND_F16 if dtype == F16 else _lib.OPERAND_BF16), rows
    a.w_scale = o["w_scale"]
    keep = [o["A"].contiguous(), W.contiguous(), bias.contiguous()]
    a.a, a.w, a.bias = ops._p(keep[0], dtype), ops._p(keep[1], dtype), ops._p(keep[2], torch.float32)
    if split:
        keep += [o["A_lo"].contiguous(), W_lo.contiguous()]
        a.a_lo, a.w_lo = ops._p(keep[-2], dtype), ops._p(keep[-1], dtype)
    if "gamma" in o:
        keep.append(o["gamma"].contiguous())
        a.gamma = ops._p(keep[-1], torch.float32)
    if ovf is not None:
        a.ovf = ops._p(ovf, torch.int32)
    out = {}
    band = 256 * N                                     # a store of a whole row tile past the last row lands here
    if o["role"] == R.QKV:
        S, Sp, heads = o["S"], o["Sp"], D // 64
        a.S, a.Sp = S, Sp
        for suf in ([""] + (["_lo"] if split else [])):
            for name in ("q", "k", "vt"):
                shp = (rows // S, heads, Sp, 64) if name != "vt" else (rows // S, heads, 64, Sp)
                out[name + suf] = Guarded(shp, dtype, heads * Sp * 64, zero=True)
                setattr(a, name + suf, out[name + suf].t.data_ptr())
    elif swiglu:
        for suf in ([""] + (["_lo"] if split else [])):
            out["out" + suf] = Guarded((rows, N), dtype, band)
            setattr(a, "out" + suf, out["out" + suf].t.data_ptr())
    elif split:
        out["x"] = Guarded((rows, N), torch.float32, band, init=o["x"])
        a.x = out["x"].t.data_ptr()
    else:
        out["out"] = Guarded((rows, N), dtype, band)
        a.out = out["out"].t.data_ptr()
    fn = lib().dtk_vit_gemm_split if split else lib().dtk_vit_gemm
    check(fn(ctypes.byref(a), ops._stream()))
    torch.cuda.synchronize()
    for name, g in out.items():
        assert g.guard_ok(), f"role {role} rows={rows}: a store past the last row of {name}"
    return {k: g.t for k, g in out.items()}


@pytest.mark.parametrize("cls", ["real", "real_outlier"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("path", list(PATHS))
def test_fc1_swiglu_vs_float64(path, dt, cls):
    flags, split, t = PATHS[path]
    dtype = F16 if dt == "fp16" else BF16
    worst = (0.0, None, None)
    for i, rows in enumerate(rows_of(t)):
        o = G.make_fc1(rows, dtype, 4001 + 97 * list(PATHS).index(path) + 13 * i + (dt == "bf16"), split=split, device=DEV,
                       outlier=cls == "real_outlier")
        got = run_stage(o, flags)
        ratio, at = G.check(o, got)
        if ratio > worst[0]:
            worst = (ratio, rows, at)
    print(f"vitg_gemm {path} {dt} {cls} fc1_swiglu: worst |got - ref| / bound = {worst[0]:.3f} at rows={worst[1]} (row, col)={worst[2]}")


def _operands(role, rows, dtype, seed, split, exact):
    if role == G.FC2_SWIGLU:
        return G.make_fc2(rows, dtype, seed, split=split, device=DEV, exact=exact)
    o = (R.make_exact if exact else R.make_real)(role, D, rows, dtype, seed, split=split, device=DEV)
    if role == R.QKV:     # one frame of 257 tokens; five frames of 157: frame ends inside the row tiles
        o["S"] = rows if rows == 257 else 157
        assert rows % o["S"] == 0
        o["Sp"] = -(-o["S"] // 64) * 64
    return o


@pytest.mark.parametrize("cls", ["exact", "real"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("path", list(PATHS))
def test_w3_qkv_proj_at_1536_vs_float64(path, dt, cls):
    flags, split, _ = PATHS[path]
    dtype = F16 if dt == "fp16" else BF16
    for role, name in ((G.FC2_SWIGLU, "fc2_swiglu"), (R.QKV, "qkv"), (R.PROJ, "proj")):
        worst = 0.0
        for i, rows in enumerate((257, 3 * 256 + 17)):
            o = _operands(role, rows, dtype, 6007 + 97 * list(PATHS).index(path) + 31 * role + 13 * i + (dt == "bf16"), split, cls == "exact")
            got = run_stage(o, flags)
            if cls == "exact":
                R.check_exact(o, got)
            elif role == G.FC2_SWIGLU:
                worst = max(worst, G.check(o, got)[0])
            else:
                worst = max(worst, R.check_real(o, got)[0])
        print(f"vitg_gemm {path} {dt} {cls} {name}: " + ("bit-equal (Q: one ulp)" if cls == "exact" else f"worst |got - ref| / bound = {worst:.3f}"))


@pytest.mark.parametrize("path", list(PATHS))
def test_swiglu_overflow_word(path):
    """ONE pair whose product leaves the fp16 range -- gate 512 (two products of 16 x 16; silu(512) = 512), value 256 -- in the last
    valid row of the last hidden column sets bit 4 and is stored as the saturated 65504; with value 127 (65024) the word stays 0;
    bf16 operands never touch the word and store 131072."""
    flags, split, t = PATHS[path]
    rows, H = 3 * t + 17, G.HIDDEN

    def craft(dtype, value):
        ws = R.W_SCALE[dtype] if split else 1.0
        o = {"role": G.FC1_SWIGLU, "D": D, "rows": rows, "dtype": dtype, "split": split, "w_scale": ws, "exact": False}
        A, W, b = torch.zeros(rows, D, device=DEV), torch.zeros(2 * H, D, device=DEV), torch.zeros(2 * H, device=DEV)
        A[rows - 1, :2] = 16.0
        W[H - 1, :2] = 16.0 * ws
        b[2 * H - 1] = value
        o["A"], o["W"], o["bias"] = A.to(dtype), W.to(dtype), b
        if split:
            o["A_lo"], o["W_lo"] = torch.zeros_like(o["A"]), torch.zeros_like(o["W"])
        return o

    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = run_stage(craft(F16, 256.0), flags, ovf=word)
    assert int(word) == 4 and float(got["out"][rows - 1, H - 1]) == 65504.0, (int(word), float(got["out"][rows - 1, H - 1]))
    assert int((got["out"] != 0).sum()) == 1
    word.zero_()
    got = run_stage(craft(F16, 127.0), flags, ovf=word)
    assert int(word) == 0 and float(got["out"][rows - 1, H - 1]) == 65024.0, (int(word), float(got["out"][rows - 1, H - 1]))
    word.fill_(0x40)
    got = run_stage(craft(BF16, 256.0), flags, ovf=word)
    assert int(word) == 0x40 and float(got["out"][rows - 1, H - 1]) == 131072.0, (int(word), float(got["out"][rows - 1, H - 1]))


def test_swiglu_stage_refusals():
    """No *_V1 form of the SwiGLU roles (the message names the flag); the roles belong to D = 1536; D = 512 is still no model width."""
    o = G.make_fc1(16, F16, 1, device=DEV)
    for flag, name in ((WIDE_V1, "DTK_VIT_GEMM_WIDE_V1"), (WS_V1, "DTK_VIT_GEMM_WS_V1")):
        with pytest.raises(RuntimeError, match=name):
            run_stage(o, flag)
        with pytest.raises(RuntimeError, match=name):
            run_stage(G.make_fc2(16, F16, 1, device=DEV), flag)
    with pytest.raises(RuntimeError, match="D = 1536"):
        run_stage(o, 0, D_arg=1024)
    with pytest.raises(RuntimeError, match="D must be"):
        run_stage(o, 0, D_arg=512)
    with pytest.raises(RuntimeError, match="unknown role"):
        run_stage(o, 0, role_arg=9)
