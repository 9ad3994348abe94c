"""CPU: the test of tests/test_gpu_vit_gemm.py's helpers (tests/vit_gemm_ref.py).  A correct GEMM -- fp32 torch.matmul of the same 16-bit
operands, the epilogue in fp32, rounding to T -- is accepted in both classes (bit-equal in the exact class: the reference alone stays
inside the bound), and each planted defect of the kind a subtly wrong kernel produces is rejected:

  * one 32-wide k-step dropped for one 32-row tile;
  * two adjacent rows swapped across a frame boundary in the Q layout;
  * the last row tile repeated from the previous one;
  * the output rounded through bf16 when T is fp16;
  * the lo x lo product included in the split sum (exact class: in the realistic class it is the MORE accurate result);
  * one element in 8192 moved by one ulp of T (exact class)."""
import pytest
import torch

import vit_gemm_ref as R

F16, BF16 = torch.float16, torch.bfloat16
D = 384
S, SP, FRAMES = 131, 192, 3     # 4-row fragments and 32-row tiles straddle the frame boundaries


def _ops(cls, role, dtype, split=False, rows=200, **kw):
    make = R.make_exact if cls == "exact" else R.make_real
    if role == R.QKV:
        rows = S * FRAMES
    o = make(role, D, rows, dtype, seed=1000 + 17 * role + (dtype == BF16) + 2 * split, split=split, **kw)
    if role == R.QKV:
        o["S"], o["Sp"] = S, SP
    return o


def _check(cls, o, got, g=None):
    if cls == "exact":
        return R.check_exact(o, got)
    return R.check_real(o, got, g)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("split", [False, True], ids=["fast", "split"])
@pytest.mark.parametrize("cls", ["exact", "real", "real_outlier"])
def test_correct_gemm_is_accepted(cls, split, dtype):
    kw = {"outlier": True} if cls == "real_outlier" else {}
    c = "exact" if cls == "exact" else "real"
    for role in (R.QKV, R.QKV_FACET, R.PROJ, R.FC1, R.FC2):
        if c == "exact" and role == R.FC1:
            continue   # GELU outputs belong to the realistic class
        o = _ops(c, role, dtype, split, **kw)
        out = _check(c, o, R.emulate(o), R.G_ERFC)
        if out:
            print(cls, "split" if split else "fast", dtype, R.ROLE_NAMES[role], "emulation ratio %.3f at %s" % out)
            # (a correctly rounded 16-bit output comes as close to 1 as a value comes to a midpoint of T: the half ulp is most of the bound)
    if not split:
        o = _ops(c, R.FC2, dtype, fused_ln=True, **kw)
        _check(c, o, R.emulate(o))


def _defect(name, o, got):
    """Plants a defect into a correct result (or recomputes it from damaged operands)."""
    role = o["role"]
    key = {R.QKV: "k", R.QKV_FACET: "out_f32"}.get(role, "x" if (o["split"] and role in (R.PROJ, R.FC2)) else "out")
    bad = {k: v.clone() for k, v in got.items()}
    if name == "k_step":
        o2 = dict(o)
        o2["A"] = o["A"].clone()
        o2["A"][32:64, 64:96] = 0
        wrong = R.emulate(o2)
        if role == R.QKV:
            return wrong   # (only rows 32..63 differ)
        bad[key][32:64] = wrong[key][32:64]
    elif name == "q_rows":
        a, b = bad["q"][0, :, S - 1].clone(), bad["q"][1, :, 0].clone()
        bad["q"][0, :, S - 1], bad["q"][1, :, 0] = b, a
    elif name == "last_tile":
        rows = o["rows"]
        t0 = rows // 32 * 32
        assert 0 < rows - t0 < 32
        bad[key][t0:rows] = bad[key][t0 - 32:rows - 32]
    elif name == "bf16":
        bad[key] = bad[key].float().to(BF16).to(F16)
    elif name == "lolo":
        return R.emulate(o, lolo=True)
    elif name == "one_ulp":
        bits = bad[key].view(torch.int16).reshape(-1)
        bits[5::8192] += 1
    return bad


DEFECTS = [
    ("k_step", R.PROJ, False), ("k_step", R.QKV, False), ("k_step", R.FC2, True), ("k_step", R.FC1, False),
    ("q_rows", R.QKV, False), ("q_rows", R.QKV, True),
    ("last_tile", R.PROJ, False), ("last_tile", R.FC2, False), ("last_tile", R.QKV_FACET, True),
    ("bf16", R.PROJ, False), ("bf16", R.FC1, False),
    ("lolo", R.QKV_FACET, True), ("lolo", R.FC2, True), ("lolo", R.QKV, True),
    ("one_ulp", R.PROJ, False), ("one_ulp", R.FC2, False),
]
DEFECT_CASES = [(n, r, sp, c, dt) for n, r, sp in DEFECTS for c in ("exact", "real") for dt in (F16, BF16)
                if not (c == "exact" and r == R.FC1)            # GELU outputs belong to the realistic class
                and not (c == "real" and n in ("lolo", "one_ulp"))   # exact class only
                and not (n == "bf16" and dt == BF16)]            # T is fp16 in this defect


@pytest.mark.parametrize("name,role,split,cls,dtype", DEFECT_CASES,
                         ids=["%s-%s-%s-%s-%s" % (n, R.ROLE_NAMES[r], "split" if sp else "fast", c, "fp16" if dt == F16 else "bf16")
                              for n, r, sp, c, dt in DEFECT_CASES])
def test_planted_defect_is_rejected(name, role, split, cls, dtype):
    o = _ops(cls, role, dtype, split)
    good = R.emulate(o)
    _check(cls, o, good, R.G_ERFC)
    bad = _defect(name, o, good)
    with pytest.raises(AssertionError):
        _check(cls, o, bad, R.G_ERFC)


def test_fused_layernorm_defects_are_rejected():
    o = _ops("exact", R.FC2, F16, fused_ln=True)
    good = R.emulate(o)
    R.check_exact(o, good)
    bad = dict(good, x=good["x"].clone())
    bad["x"][7, 11] += 2.0 ** -10          # an fp32 ulp or so of x
    with pytest.raises(AssertionError):
        R.check_exact(o, bad)
    bad = dict(good, ln_out=good["ln_out"].clone())
    bad["ln_out"].view(torch.int16)[3, 5] += 2
    with pytest.raises(AssertionError):
        R.check_exact(o, bad)


def test_padding_rows_are_checked():
    o = _ops("exact", R.QKV, F16)
    bad = R.emulate(o)
    bad["vt"][1, 2, 3, S] = 1.0
    with pytest.raises(AssertionError, match="padding"):
        R.check_exact(o, bad)


def test_ulp_and_grid_helpers():
    x = torch.tensor([0.0, 1.0, 1.5, 2.0, 2.0 ** -14, 2.0 ** -20, 65504.0, 3.0e38], dtype=torch.float64)
    assert R.ulp(x, F16).tolist()[:7] == [2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 32.0]
    assert R.ulp(x, BF16).tolist()[1:4] == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6]
    for v in (0.3, 7.0, 1000.0, 6e-6):
        t = torch.tensor([v], dtype=torch.float64)
        for dt in (F16, BF16):
            a = t.float().to(dt)
            nxt = (a.view(torch.int16) + 1).view(dt)
            assert float(nxt.double() - a.double()) == float(R.ulp(a.double(), dt)), (v, dt)
    # csrc/vit_gemm_ws.h gemm_ws_grid: the projection runs one tile per chunk up to 4096 rows, the QKV GEMM up to 1632
    assert R.ws_grid(384, 4096)[1] == 1 and R.ws_grid(384, 4097)[1] == 2
    assert R.ws_grid(1152, 1632)[1] == 1 and R.ws_grid(1152, 1633)[1] == 2
    for N in (384, 1152, 1536):
        for lo, hi in ((2, 2), (3, 3), (5, 99)):
            rows = R.ws_rows_for(N, lo, hi)
            nch, tpc, last = R.ws_grid(N, rows)
            assert lo <= tpc <= hi and nch > 1 and 0 < last < tpc and rows % 32
    rows = R.ws_rows_for(1152, 2, 2, step=222)
    assert rows % 222 == 0 and R.ws_grid(1152, rows)[1] == 2
