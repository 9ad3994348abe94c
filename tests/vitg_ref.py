"""ViT-g/14 (upstream vit_giant2: D = 1536, 40 blocks, 24 heads, SwiGLUFFNFused with hidden 4096) -- the reference of the tests that
cover it: tests/test_vitg_reference.py (CPU), tests/test_gpu_vitg_gemm.py and tests/test_gpu_vitg.py.

* The block and the encoder restated in plain torch (float64 when the inputs are): oracle.ref_algo.vit_block is the GELU block and
  stays so; the SwiGLU feed-forward is, from the published definition,
      x1, x2 = w12(x).chunk(2, -1);   y = w3(silu(x1) * x2),   silu(v) = v / (1 + exp(-v)).
* The row interleave of w12 / b12 that the device's epilogue expects (include/dtk.h, dtk_vit_model.ffn), written here as an index
  table -- independently of VitExtractor's reshape.
* Operands, float64 reference and per-element bound of the two stage roles the model adds (dtk_vit_gemm: FC1_SWIGLU, FC2_SWIGLU), in
  the conventions of tests/vit_gemm_ref.py (imported as R; its classes (a) EXACT and (b) REALISTIC).

The SwiGLU bound.  With a = pre1 (gate), b = pre2 (value) in float64 on the operands the device read and
acc_i = C_ACC K 2^-24 mag_i (mag_i = |A| @ |W_i|^T + |bias_i|; split operands: plus the dropped lo x lo term 2^-22 / 2^-16 |A| @ |W_i|^T):

    |got - silu(a) b| <= first + 1.10 acc_1 |b| + |silu(a)| acc_2 + acc_1 acc_2 + g_silu(a) |b|

1.10 bounds sup |silu'| = 1.0998; `first` is R.bound's: half an ulp of T for a 16-bit output, 2^-22 |ref| (fp16, never below 2^-25) /
2^-16 |ref| (bf16) for hi + lo planes.  g_silu is the evaluation error of the device's silu, from the source comment next to it
(csrc/vit_gemm_common.h, silu_f32): 4e-7 * max(1, |v|).  It is stated relative to max(1, |v|) because no absolute constant can
hold at |v| = 1e4, where one fp32 ulp of the result is already 9.8e-4; below |v| = 1 it IS the absolute 4e-7.
"""
import re
from pathlib import Path

import torch
import torch.nn.functional as F

import vit_gemm_ref as R
from oracle import ref_algo

D_G, HIDDEN, HEADS, DEPTH = 1536, 4096, 24, 40
FC1_SWIGLU, FC2_SWIGLU = 5, 6            # dtk_vit_gemm_args.role (dino_tracker_amd._lib.VIT_GEMM_FC?_SWIGLU)
GROUP = 32                               # the interleave group
SILU_LIP = 1.10
G_SILU = 4e-7                            # x max(1, |v|); test_vitg_reference.py checks that the source comment says the same


def g_silu_from_source():
    """The number the kernel's source comment states: `SILU_ERR: |silu~(v) - silu(v)| <= <number> * max(1, |v|)`."""
    src = (Path(__file__).resolve().parents[1] / "dino_tracker_amd" / "csrc" / "vit_gemm_common.h").read_text()
    m = re.search(r"SILU_ERR:[^\n]*<=\s*([0-9.eE+-]+)\s*\*\s*max\(1, \|v\|\)", src)
    assert m, "csrc/vit_gemm_common.h: the SILU_ERR comment is gone"
    return float(m.group(1))


def silu64(v):
    return v * torch.sigmoid(v)          # float64 in, float64 out: torch's sigmoid has no cancellation in either tail


def silu_device_f32(v32):
    """silu_f32 of csrc/vit_gemm_common.h operation by operation in fp32: e = exp2(v * -log2(e)); v * (1 / (1 + e)).  torch's exp2 and
    reciprocal are correctly rounded to within an ulp like v_exp_f32 / v_rcp_f32; overflow of e to +inf gives v * 0."""
    assert v32.dtype == torch.float32
    e = torch.exp2(v32 * torch.tensor(-1.4426950408889634, dtype=torch.float32))
    return v32 * (1.0 / (1.0 + e))


# ---- the packed layout ----------------------------------------------------------------------------------------------------------------
def pack_index(hidden=HIDDEN, group=GROUP):
    """src[p] = the w12 row that packed row p holds: packed rows 64 g .. 64 g + 31 are gate rows 32 g .., packed rows 64 g + 32 ..
    64 g + 63 are value rows hidden + 32 g ..  Built row by row (VitExtractor builds it by reshape / stack)."""
    src = []
    for p in range(2 * hidden):
        g, i = divmod(p, 2 * group)
        src.append(group * g + i if i < group else hidden + group * g + (i - group))
    return torch.tensor(src, dtype=torch.long)


def pack_rows(t, hidden=HIDDEN):
    """w12 [2 hidden][...] or b12 [2 hidden] -> the packed order."""
    return t[pack_index(hidden).to(t.device)].contiguous()


# ---- the block and the encoder ----------------------------------------------------------------------------------------------------------
def swiglu_ffn(y, sd, p):
    x12 = F.linear(y, sd[p + "mlp.w12.weight"], sd[p + "mlp.w12.bias"])
    x1, x2 = x12.chunk(2, dim=-1)
    return F.linear(x1 * torch.sigmoid(x1) * x2, sd[p + "mlp.w3.weight"], sd[p + "mlp.w3.bias"])


def vitg_block(x, sd, i, heads=HEADS, return_qkv=False):
    """DINOv2 block at eval with the SwiGLU feed-forward: x += g1 proj(MHSA(LN1 x)); x += g2 w3(silu(x1) x2); LN eps 1e-6."""
    p = f"blocks.{i}."
    b, s, d = x.shape
    y = F.layer_norm(x, (d,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps=1e-6)
    qkv_flat = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
    q, k, v = qkv_flat.reshape(b, s, 3, heads, d // heads).permute(2, 0, 3, 1, 4)
    a = torch.softmax((q @ k.transpose(-1, -2)) * (q.shape[-1] ** -0.5), dim=-1) @ v
    a = a.transpose(1, 2).reshape(b, s, d)
    x = x + sd[p + "ls1.gamma"] * F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    y = F.layer_norm(x, (d,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps=1e-6)
    out = x + sd[p + "ls2.gamma"] * swiglu_ffn(y, sd, p)
    return (out, qkv_flat) if return_qkv else out


def vitg_tokens(frames, sd, layer, stride=7, patch=14, normalize=True, return_qkv=False, taps=None):
    """VitExtractor.get_feature_from_input for frames [B,3,H,W]: the output of block `layer` (-1: embedding only), [B, 1 + ph*pw, D], in
    the dtype of frames / sd (float64 for the reference, float32 for the fp32 yardstick).  taps: the mean of those blocks' outputs."""
    x = frames
    if normalize:
        m = torch.tensor(ref_algo.IMAGENET_MEAN, dtype=frames.dtype).view(1, 3, 1, 1)
        s = torch.tensor(ref_algo.IMAGENET_STD, dtype=frames.dtype).view(1, 3, 1, 1)
        x = (x - m) / s
    ph, pw = ref_algo.feature_grid(frames.shape[-2], frames.shape[-1], patch, stride)
    tok = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=stride)
    tok = tok.flatten(2).transpose(1, 2)
    tok = torch.cat([sd["cls_token"].expand(tok.shape[0], -1, -1), tok], dim=1) + ref_algo.vit_pos_embed(sd, ph, pw)
    qkv, acc = None, None
    for i in range(layer + 1):
        tok, qkv = vitg_block(tok, sd, i, return_qkv=True)
        if taps is not None and i in taps:
            acc = tok / len(taps) if acc is None else acc + tok / len(taps)
    if taps is not None:
        return acc
    return (tok, qkv) if return_qkv else tok


def to64(sd):
    return {k: v.double() for k, v in sd.items()}


# ---- stage operands -------------------------------------------------------------------------------------------------------------------
def _planes(x32, dtype, split):
    hi = x32.to(dtype)
    return (hi, (x32 - hi.float()).to(dtype)) if split else (hi, None)


def make_fc1(rows, dtype, seed, split=False, device="cpu", outlier=False, exact_sums=False):
    """Class (b) operands of the w12 GEMM in UNPACKED row order (gate rows 0 .. 4095, value rows 4096 ..): LayerNorm-like activations
    with three outlier channels (R.make_real's), weights N(0, 0.04), bias N(0, 0.02); `outlier`: LayerNorm gains up to 8.
    exact_sums (split planes only): R.make_exact's integer planes, so that the three-product sums hh + hl + lh are exact in fp32 in
    any order and only the epilogue is left to bound -- the class in which a FOURTH product shows (bound_fc1)."""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)   # noqa: E731
    if exact_sums:
        assert split
        ints = lambda s, r: torch.randint(-r, r + 1, s, generator=g, device=device).float()   # noqa: E731
        r, sh = (3 if dtype == torch.float16 else 2), 2.0 ** -R.LO_SHIFT[dtype]
        return {"role": FC1_SWIGLU, "D": D_G, "rows": rows, "dtype": dtype, "split": True, "exact": True, "w_scale": R.W_SCALE[dtype],
                "A": ints((rows, D_G), r).to(dtype), "W": ints((2 * HIDDEN, D_G), r).to(dtype),
                "A_lo": (ints((rows, D_G), r) * sh).to(dtype), "W_lo": (ints((2 * HIDDEN, D_G), r) * sh).to(dtype),
                "bias": ints((2 * HIDDEN,), 4) / 64.0}
    A = rn(rows, D_G)
    A[:, torch.randperm(D_G, generator=g, device=device)[:3]] *= 30.0
    if outlier:
        A = A * (1.0 + 7.0 * torch.rand(D_G, generator=g, device=device) ** 4)
    W = rn(2 * HIDDEN, D_G) * 0.04
    o = {"role": FC1_SWIGLU, "D": D_G, "rows": rows, "dtype": dtype, "split": split, "exact": False, "bias": rn(2 * HIDDEN) * 0.02,
         "w_scale": R.W_SCALE[dtype] if split else 1.0}
    o["A"], a_lo = _planes(A, dtype, split)
    o["W"], w_lo = _planes(W * o["w_scale"], dtype, split)
    if split:
        o["A_lo"], o["W_lo"] = a_lo, w_lo
    return o


def make_fc2(rows, dtype, seed, split=False, device="cpu", outlier=False, exact=False):
    """Operands of the w3 GEMM (N = 1536, K = 4096) as a dict that vit_gemm_ref treats as its FC2 role (`role_dev` is what the device is
    given).  exact: R.make_exact's integer class; otherwise a SwiGLU hidden -- silu of a Gaussian times a Gaussian, three outlier
    channels -- against weights N(0, 0.03) (outlier: x 300, LayerScale up to 3), as R.make_real draws fc2."""
    N, K = D_G, HIDDEN
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)   # noqa: E731
    ints = lambda s, r: torch.randint(-r, r + 1, s, generator=g, device=device).float()   # noqa: E731
    o = {"role": R.FC2, "role_dev": FC2_SWIGLU, "D": D_G, "rows": rows, "dtype": dtype, "split": split, "exact": exact,
         "w_scale": R.W_SCALE[dtype] if split else 1.0}
    if exact:
        if split:
            r, sh = (3 if dtype == torch.float16 else 2), 2.0 ** -R.LO_SHIFT[dtype]
            o["A"], o["W"] = ints((rows, K), r).to(dtype), ints((N, K), r).to(dtype)
            o["A_lo"], o["W_lo"] = (ints((rows, K), r) * sh).to(dtype), (ints((N, K), r) * sh).to(dtype)
            o["bias"] = ints((N,), 4)
        else:
            o["A"], o["W"], o["bias"] = ints((rows, K), 8).to(dtype), ints((N, K), 4).to(dtype), ints((N,), 16)
        mag = torch.tensor([0.5, 1.0, 2.0], device=device)[torch.randint(0, 3, (N,), generator=g, device=device)]
        o["gamma"] = mag * (torch.randint(0, 2, (N,), generator=g, device=device).float() * 2 - 1)
        if split:
            o["x"] = ints((rows, N), 64)
        return o
    A = (silu64((1.5 * rn(rows, K)).double()) * rn(rows, K).double()).float()
    A[:, torch.randperm(K, generator=g, device=device)[:3]] *= 30.0
    W = rn(N, K) * 0.03 * (300.0 if outlier else 1.0)
    o["bias"] = rn(N) * 0.02
    o["A"], a_lo = _planes(A, dtype, split)
    o["W"], w_lo = _planes(W * o["w_scale"], dtype, split)
    o["gamma"] = (1.0 + 0.1 * rn(N)) * ((0.5 * (1.0 + 5.0 * torch.rand(N, generator=g, device=device) ** 4)) if outlier else 1.0)
    if split:
        o["A_lo"], o["W_lo"], o["x"] = a_lo, w_lo, 3.0 * rn(rows, N)
    return o


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------
def _first(ref, dtype, split):
    if split:
        return (2.0 ** -22 * ref.abs()).clamp(min=2.0 ** -25) if dtype == torch.float16 else 2.0 ** -16 * ref.abs()
    return 0.5 * R.ulp(ref, dtype)


def bound_fc1(o):
    """(ref, bound) of the SwiGLU stage, float64 [rows][4096] (module docstring)."""
    r = R.reference(o)
    K = o["A"].shape[1]
    pre = r["pre"]
    if o["exact"]:
        # integer planes: the kernel's sum hh + hl + lh is exact (asserted as R.check_exact does), its division by the power-of-two
        # w_scale too; the bias add rounds once.  The reference is that three-product sum -- lo x lo must NOT be in it
        unit = 2.0 ** -R.LO_SHIFT[o["dtype"]] / o["w_scale"]
        assert float((r["mag"] - r["lolo"]).max()) / unit < 2.0 ** 24
        pre, acc = r["pre3"], R.U32 * r["mag"]
    else:
        acc = R.C_ACC * K * R.U32 * r["mag"]
        if o["split"]:
            acc = acc + (2.0 ** -22 if o["dtype"] == torch.float16 else 2.0 ** -16) * r["absAW"]
    a, b = pre[:, :HIDDEN], pre[:, HIDDEN:]
    a1, a2 = acc[:, :HIDDEN], acc[:, HIDDEN:]
    s = silu64(a)
    ref = s * b
    g = G_SILU * a.abs().clamp(min=1.0)
    return ref, _first(ref, o["dtype"], o["split"]) + SILU_LIP * a1 * b.abs() + s.abs() * a2 + a1 * a2 + g * b.abs()


def bound_fc2(o):
    """(ref, bound) of the w3 stage: R.bound's residual-update case with K read from the operands (R.shape knows 4 D only)."""
    r = R.reference(o)
    K = o["A"].shape[1]
    sc = o["gamma"].double()
    ref = r["pre"] * sc
    acc = R.C_ACC * K * R.U32 * r["mag"] * sc.abs()
    if o["split"]:
        ref = o["x"].double() + ref
        first = R.U32 * ref.abs() + (2.0 ** -22 if o["dtype"] == torch.float16 else 2.0 ** -16) * r["absAW"] * sc.abs()
    else:
        first = 0.5 * R.ulp(ref, o["dtype"])
    return ref, first + acc


def hidden64(o, got):
    m = got["out"].double()
    return m + got["out_lo"].double() if o["split"] else m


def check(o, got):
    """Largest |got - ref| / bound and where; raises beyond 1 or on a non-finite output."""
    if o["role"] == FC1_SWIGLU:
        (ref, b), g = bound_fc1(o), hidden64(o, got)
    else:
        (ref, b), g = bound_fc2(o), R.matrix(o, got).double()
    assert bool(torch.isfinite(g).all()), "non-finite output"
    ratio = (g - ref).abs() / b
    worst = float(ratio.max())
    at = divmod(int(ratio.argmax()), ratio.shape[1])
    assert worst <= 1.0, (f"role {o.get('role_dev', o['role'])}: |got - ref| / bound = {worst:.3f} at (row, col) {at}", float(g[at]), float(ref[at]), float(b[at]))
    return worst, at


# ---- an emulation of a correct kernel, and of wrong ones ---------------------------------------------------------------------------------
def emulate_fc1(o, defect=None):
    """fp32 matmul of the operands the device reads, bias, silu (through float64, rounded to fp32: its approximation is test (iv)'s
    subject), the product in fp32, rounding to T / hi + lo planes.  defect: "silu_on_value", "no_bias_value", "pair_shift" (gate j
    meets the value of the next interleave group), "lolo" (a fourth product in the split sum)."""
    dtype, H = o["dtype"], HIDDEN
    bias = o["bias"].float().clone()
    if defect == "no_bias_value":
        bias[H:] = 0.0
    if o["split"]:
        Ah, Al, Wh, Wl = o["A"].float(), o["A_lo"].float(), o["W"].float(), o["W_lo"].float()
        acc = Ah @ Wl.T + Al @ Wh.T
        if defect == "lolo":
            acc = acc + Al @ Wl.T
        v = (acc + Ah @ Wh.T) * (1.0 / o["w_scale"]) + bias
    else:
        v = o["A"].float() @ o["W"].float().T + bias
    gate, value = v[:, :H], v[:, H:]
    if defect == "pair_shift":
        value = torch.roll(value, -GROUP, dims=1)
    if defect == "silu_on_value":
        gate, value = value, gate
    u = silu64(gate.double()).float() * value
    hi, lo = _planes(u, dtype, o["split"])
    return {"out": hi, "out_lo": lo} if o["split"] else {"out": hi}
