"""-m gpu: every GEMM kernel of the ViT encoder ALONE (dtk_vit_gemm / dtk_vit_gemm_split: the dispatch of dtk_vit_forward for a model
width and flag set, one role at a time) against float64 on the operands the device read -- which output element of which GEMM is
wrong, with a tolerance that comes from the arithmetic (tests/vit_gemm_ref.py: the exact class has none; its CPU counterpart,
tests/test_vit_gemm_reference.py, shows that the checks reject a subtly wrong kernel).

Paths (D, flags) -> kernels, per csrc/vit.hip launch_gemm / launch_gemm_split:
  vits          384, 0            gemm_ws_kernel (qkv, proj, fc1), gemm_wide_delta_kernel<T, true> (fc2), <T, true, true> (fc2 + LayerNorm)
  vits_ws_v1    384, GEMM_WS_V1   gemm_ws_kernel<T, EPI, 0>
  vits_wide_v1  384, GEMM_WIDE_V1 gemm_wide_delta_kernel<T, false> (fc2)
  vits_tiled    384, TILED_GEMMS  gemm_tiled_kernel, every role and the fp32 facet
  vitb / vitl   768 / 1024, 0     gemm_wide_kernel<T, EPI, true>;  ..._wide_v1: <T, EPI, false>
  split_*       384 / 1024        gemm_split_dma_kernel<T, SEPI, true> (0), <..., false> (GEMM_WIDE_V1), gemm_split_kernel (TILED_GEMMS)
Row counts come from the kernels' tiles (t = 32 weight-stationary, 128 tiled, 256 LDS-DMA): 1, t - 1, t, t + 1, 3 t + 17; more than
8 x 256 rows with a ragged last block for the `(kb / ncol) * 8 + (blockIdx.x & 7)` swizzle; for the weight-stationary kernel the
counts that give 2, 3 and >= 5 token tiles per chunk with a short last chunk (gemm_ws_grid; asserted).  QKV runs frames of S
tokens whose boundaries cut 4-row fragments and 32-row tiles (S = 222 x 3, 131 x 5), S = 132 x 4 for the 8-byte V^T stores and
S = 21 x 7 -- frames shorter than a 32-row tile, several frame ends inside one tile.
Every output has a guard band behind its last row that must come back untouched, and unwritten elements hold a sentinel.

Every case prints its largest |got - ref| / bound and where it occurs; the record of those figures: docs/PARITY.md ("GEMM stages"),
docs/MEASUREMENTS.md."""
import ctypes

import pytest
import torch

import vit_gemm_ref as R
from dino_tracker_amd import _lib, ops
from dino_tracker_amd._lib import check, lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A
TILED, WS_V1, WIDE_V1 = _lib.VIT_TILED_GEMMS, _lib.VIT_GEMM_WS_V1, _lib.VIT_GEMM_WIDE_V1
assert (R.QKV, R.QKV_FACET, R.PROJ, R.FC1, R.FC2) == (_lib.VIT_GEMM_QKV, _lib.VIT_GEMM_QKV_FACET, _lib.VIT_GEMM_PROJ, _lib.VIT_GEMM_FC1,
                                                      _lib.VIT_GEMM_FC2)
FUSED = "fc2+ln"   # pseudo-role: fc2 with the next block's LayerNorm in its epilogue

# name: (D, flags, split, roles)
PATHS = {
    "vits": (384, 0, False, [R.QKV, R.PROJ, R.FC1, R.FC2, FUSED]),
    "vits_ws_v1": (384, WS_V1, False, [R.QKV, R.PROJ, R.FC1]),
    "vits_wide_v1": (384, WIDE_V1, False, [R.FC2]),
    "vits_tiled": (384, TILED, False, [R.QKV, R.QKV_FACET, R.PROJ, R.FC1, R.FC2]),
    "vitb": (768, 0, False, [R.QKV, R.PROJ, R.FC1, R.FC2]),
    "vitb_wide_v1": (768, WIDE_V1, False, [R.QKV, R.PROJ, R.FC1, R.FC2]),
    "vitl": (1024, 0, False, [R.QKV, R.PROJ, R.FC1, R.FC2]),
    "vitl_wide_v1": (1024, WIDE_V1, False, [R.QKV, R.PROJ, R.FC1, R.FC2]),
    "split_vits": (384, 0, True, [R.QKV, R.QKV_FACET, R.PROJ, R.FC1, R.FC2]),
    "split_vits_wide_v1": (384, WIDE_V1, True, [R.QKV, R.QKV_FACET, R.FC1, R.FC2]),
    "split_vits_tiled": (384, TILED, True, [R.QKV, R.QKV_FACET, R.PROJ, R.FC1, R.FC2]),
    "split_vitl": (1024, 0, True, [R.QKV, R.QKV_FACET, R.FC1, R.FC2]),
    "split_vitl_wide_v1": (1024, WIDE_V1, True, [R.QKV, R.QKV_FACET, R.FC1, R.FC2]),
    "split_vitl_tiled": (1024, TILED, True, [R.QKV, R.QKV_FACET, R.FC1, R.FC2]),
}


def family(D, flags, split, role):
    """(kernel family, row tile, documented GELU error) of a role on a path: the table of launch_gemm / launch_gemm_split."""
    if split:
        return ("split_tiled", 128, R.G_ERFC) if flags & TILED else ("split_dma", 256, R.G_ERFC)
    if flags & TILED or role == R.QKV_FACET:
        return "tiled", 128, "erff"
    if D == 384:
        return ("wide_delta", 256, None) if role == R.FC2 else ("ws", 32, R.G_GELU2)
    return "wide", 256, R.G_GELU2


def row_cases(D, flags, split, role):
    """[(rows, S, Sp)] for a role on a path (module docstring); S = 0 outside QKV."""
    fam, t, _ = family(D, flags, split, role)
    N, _ = R.shape(role, D)
    sp = lambda s: -(-s // 64) * 64   # noqa: E731
    rows = [1, t - 1, t, t + 1, 3 * t + 17]
    if role != R.QKV:
        if fam in ("wide", "wide_delta", "split_dma"):
            rows.append(8 * 256 + 256 + 77)              # 10 row blocks: the second swizzle group, ragged
        if fam == "ws":
            for lo, hi in ((2, 2), (3, 3), (5, 99)):
                r = R.ws_rows_for(N, lo, hi)
                nch, tpc, last = R.ws_grid(N, r)
                assert lo <= tpc <= hi and nch > 1 and 0 < last < tpc, (N, r, nch, tpc, last)
                rows.append(r)
            if N == 384:
                assert rows[-3] > 4096                   # the projection leaves one tile per chunk only beyond 4096 rows
        return [(r, 0, 0) for r in rows]
    cases = [(r, r, sp(r)) for r in rows] + [(3 * 222, 222, 256), (5 * 131, 131, 192), (4 * 132, 132, 192), (7 * 21, 21, 64)]
    if fam in ("wide", "split_dma"):
        cases.append((11 * 222, 222, 256))               # 2442 rows: 10 row blocks
    if fam == "ws":
        for lo, hi, s in ((2, 2, 222), (3, 3, 131), (5, 99, 222)):
            r = R.ws_rows_for(N, lo, hi, step=s)
            nch, tpc, last = R.ws_grid(N, r)
            assert lo <= tpc <= hi and nch > 1 and 0 < last < tpc and r % s == 0, (N, r, nch, tpc, last)
            cases.append((r, s, sp(s)))
    return cases


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


def run_stage(o, flags, fused=False, ovf=None):
    """One launch of the stage on the operands `o` (tests/vit_gemm_ref.py); returns the outputs in the stage's layouts."""
    role, D, dtype, split, rows = o["role"], o["D"], o["dtype"], o["split"], o["rows"]
    N, K = R.shape(role, D)
    a = _lib.VitGemmArgs()
    a.role, a.D, a.flags, a.operand_type, a.rows = role, D, flags, (_lib.OPERAND_F16 if dtype == F16 else _lib.OPERAND_BF16), rows
    a.w_scale = o["w_scale"]
    keep = [o["A"].contiguous(), o["W"].contiguous(), o["bias"].contiguous()]
    a.a, a.w, a.bias = ops._p(keep[0], dtype), ops._p(keep[1], dtype), ops._p(keep[2], torch.float32)
    if split:
        keep += [o["A_lo"].contiguous(), o["W_lo"].contiguous()]
        a.a_lo, a.w_lo = ops._p(keep[-2], dtype), ops._p(keep[-1], dtype)
    if "gamma" in o:
        keep.append(o["gamma"].contiguous())
        a.gamma = ops._p(keep[-1], torch.float32)
    if ovf is not None:
        a.ovf = ops._p(ovf, torch.int32)
    out = {}
    band = 256 * N                                     # a store of a whole row tile past the last row lands here
    if role == R.QKV:
        S, Sp, heads = o["S"], o["Sp"], D // 64
        a.S, a.Sp = S, Sp
        F = rows // S
        for suf in ([""] + (["_lo"] if split else [])):
            for name in ("q", "k", "vt"):
                shp = (F, heads, Sp, 64) if name != "vt" else (F, heads, 64, Sp)
                out[name + suf] = Guarded(shp, dtype, heads * Sp * 64, zero=True)   # guard: one more frame
                setattr(a, name + suf, out[name + suf].t.data_ptr())
    elif role == R.QKV_FACET:
        out["out_f32"] = Guarded((rows, N), torch.float32, band)
        a.out_f32 = out["out_f32"].t.data_ptr()
    elif role == R.FC1:
        for suf in ([""] + (["_lo"] if split else [])):
            out["out" + suf] = Guarded((rows, N), dtype, band)
            setattr(a, "out" + suf, out["out" + suf].t.data_ptr())
    elif split:
        out["x"] = Guarded((rows, N), torch.float32, band, init=o["x"])
        a.x = out["x"].t.data_ptr()
    else:
        out["out"] = Guarded((rows, N), dtype, band)     # (the fused form must leave it alone: checked below)
        a.out = out["out"].t.data_ptr()
        if fused:
            out["x"] = Guarded((rows, N), torch.float32, band, init=o["x"])
            out["ln_out"] = Guarded((rows, N), dtype, band)
            keep += [o["ln_w"].contiguous(), o["ln_b"].contiguous()]
            a.ln_x, a.ln_out, a.ln_w, a.ln_b, a.ln_eps = out["x"].t.data_ptr(), out["ln_out"].t.data_ptr(), ops._p(keep[-2]), ops._p(keep[-1]), o["ln_eps"]
    fn = lib().dtk_vit_gemm_split if split else lib().dtk_vit_gemm
    check(fn(ctypes.byref(a), ops._stream()))
    torch.cuda.synchronize()
    for name, g in out.items():
        assert g.guard_ok(), f"{R.ROLE_NAMES[role]} rows={rows}: a store past the last row of {name}"
    if fused:
        untouched = out.pop("out")
        assert bool((untouched.flat == SENT16).all()), "the fused form stored the update as well"
    return {k: g.t for k, g in out.items()}


def launch_name(role, split):
    return "vit_gemm_" + R.ROLE_NAMES[role] + ("_split" if split and role != R.QKV_FACET else "")


@pytest.mark.parametrize("cls", ["exact", "real", "real_outlier"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("path", list(PATHS))
def test_gemm_stage_vs_float64(path, dt, cls):
    """Every role of a path at every row count of its kernel family, against float64 on the same operands: bit equality in the exact
    class (Q: one ulp), the derived per-element bound in the realistic one.  Prints the largest |got - ref| / bound of each role and
    where it occurs; asserts from the profile's launch names and counts that every case was launched.  (real_outlier: the
    outlier statistics of synth.make_outlier_vit_weights, at the two largest row counts of each role.)"""
    D, flags, split, roles = PATHS[path]
    dtype = F16 if dt == "fp16" else BF16
    exact = cls == "exact"
    ops.profile_enable(True)
    launched = {}
    try:
        for role_ in roles:
            fused = role_ == FUSED
            role = R.FC2 if fused else role_
            if exact and role == R.FC1:
                continue                                   # GELU outputs belong to the realistic class
            _, _, gelu_g = family(D, flags, split, role)
            cases = row_cases(D, flags, split, role)
            if cls == "real_outlier":
                cases = cases[-2:]
            worst = (0.0, None, None)
            for i, (rows, S, Sp) in enumerate(cases):
                seed = 7919 * (1 + list(PATHS).index(path)) + 101 * role + 13 * i + (dt == "bf16")
                kw = dict(split=split, device=DEV, fused_ln=fused)
                o = R.make_exact(role, D, rows, dtype, seed, **kw) if exact else R.make_real(role, D, rows, dtype, seed, outlier=cls == "real_outlier", **kw)
                if role == R.QKV:
                    o["S"], o["Sp"] = S, Sp
                got = run_stage(o, flags, fused=fused)
                launched[launch_name(role, split)] = launched.get(launch_name(role, split), 0) + 1
                if exact:
                    R.check_exact(o, got)
                    if fused:   # the same inputs through the unfused form: the exact-class delta
                        o2 = {k: v for k, v in o.items() if k not in ("x", "ln_w", "ln_b", "ln_eps")}
                        R.check_exact(o2, run_stage(o2, flags))
                        launched["vit_gemm_fc2"] += 1
                else:
                    ratio, at = R.check_real(o, got, gelu_g)
                    if ratio > worst[0]:
                        worst = (ratio, rows, at)
            name = FUSED if fused else R.ROLE_NAMES[role]
            if exact:
                print(f"vit_gemm {path} {dt} exact {name}: {len(cases)} row counts bit-equal (Q: one ulp)")
            else:
                print(f"vit_gemm {path} {dt} {cls} {name}: worst |got - ref| / bound = {worst[0]:.3f} at rows={worst[1]} (row, col)={worst[2]}")
        prof = ops.profile_collect()
        for name, n in launched.items():
            assert name in prof and prof[name][1] == n, (name, n, prof.get(name))
        assert set(prof) == set(launched), (sorted(prof), sorted(launched))
    finally:
        ops.profile_enable(False)


OVF_PATHS = ["vits", "vits_ws_v1", "vits_tiled", "vitb", "vitb_wide_v1", "split_vits", "split_vits_wide_v1", "split_vits_tiled"]


@pytest.mark.parametrize("role", [R.QKV, R.FC1], ids=["qkv", "fc1"])
@pytest.mark.parametrize("path", OVF_PATHS)
def test_overflow_word(path, role):
    """The fp16 range word (GemmEpi::ovf / SplitEpi::ovf): ONE stored value of 65536 >= 65488 -- finite operands, 256 products of
    16 x 16 -- in the last valid row of the last column group sets bit 2 (QKV) / 4 (fc1) and is stored as the saturated 65504; with
    255 products (65280) the word stays 0; with bf16 operands the word is never touched; a pre-activation of -65536 in fc1 does not
    set the bit (GELU stores ~0 there: the epilogues track the positive part) -- and what is stored there is checked too."""
    D, flags, split, _ = PATHS[path]
    N, K = R.shape(role, D)
    _, t, _ = family(D, flags, split, role)
    S = 3 * t + 17
    rows = S
    bit = 2 if role == R.QKV else 4

    def craft(dtype, terms, sign=1.0):
        ws = R.W_SCALE[dtype] if split else 1.0
        o = {"role": role, "D": D, "rows": rows, "dtype": dtype, "split": split, "w_scale": ws, "exact": False, "S": S, "Sp": -(-S // 64) * 64}
        A, W = torch.zeros(rows, K, device=DEV), torch.zeros(N, K, device=DEV)
        A[rows - 1, :terms] = 16.0 * sign
        W[N - 1, :256] = 16.0 * ws
        o["A"], o["W"], o["bias"] = A.to(dtype), W.to(dtype), torch.zeros(N, device=DEV)
        if split:
            o["A_lo"], o["W_lo"] = torch.zeros_like(o["A"]), torch.zeros_like(o["W"])
        return o

    def stored(o, got):
        return float(R.matrix(o, got)[rows - 1, N - 1])

    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    o = craft(F16, 256)
    got = run_stage(o, flags, ovf=word)
    assert int(word) == bit and stored(o, got) == 65504.0, (int(word), stored(o, got))
    word.zero_()
    o = craft(F16, 255)
    got = run_stage(o, flags, ovf=word)
    assert int(word) == 0 and stored(o, got) == 65280.0, (int(word), stored(o, got))
    if role == R.FC1:
        # GELU(-65536) = 0.  gelu2 (weight-stationary and wide kernels) clamps its argument to +-4.25, where its erf polynomial is
        # documented to |error| < 2e-5: it returns x / 2 * (1 + erf~(-4.25 / sqrt 2)), at most |x| / 2 * 2e-5 = 0.66 in magnitude
        # (MI355X: -0.3145); the erff / erfc forms return a zero.
        got = run_stage(craft(F16, 256, -1.0), flags, ovf=word)
        limit = 65536.0 / 2 * 2e-5 if family(D, flags, split, role)[2] == R.G_GELU2 else 0.0
        assert int(word) == 0 and abs(stored(o, got)) <= limit, (int(word), stored(o, got))
    word.fill_(0x40)
    o = craft(BF16, 256)
    got = run_stage(o, flags, ovf=word)
    assert int(word) == 0x40 and stored(o, got) == 65536.0, (int(word), stored(o, got))


def test_stage_refuses_bad_arguments():
    """dtk_vit_gemm validates what it is given the way dtk_vit_attention does (error code + message, nothing launched)."""
    o = R.make_exact(R.FC2, 384, 64, F16, 1, device=DEV, fused_ln=True)
    a = _lib.VitGemmArgs()
    for D, role, want in ((512, R.PROJ, b"D must be"), (384, 9, b"unknown role")):
        a.role, a.D, a.rows, a.a, a.w = role, D, 64, o["A"].data_ptr(), o["W"].data_ptr()
        assert lib().dtk_vit_gemm(ctypes.byref(a), None) == -1 and want in lib().dtk_last_error()
    with pytest.raises(RuntimeError, match="fused LayerNorm"):
        run_stage(o, TILED, fused=True)
    o = R.make_exact(R.QKV, 384, 100, F16, 1, device=DEV)
    o["S"], o["Sp"] = 33, 64                              # rows is not a multiple of S
    with pytest.raises(RuntimeError, match="bad sizes"):
        run_stage(o, 0)
