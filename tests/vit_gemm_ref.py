"""Expected values and error bounds for ONE GEMM of a ViT block (dtk_vit_gemm / dtk_vit_gemm_split, include/dtk.h), shared by
tests/test_gpu_vit_gemm.py (the kernels) and tests/test_vit_gemm_reference.py (a CPU emulation and planted defects: the test of
the test).  Everything here is plain torch in float64 on the operands the device read -- the 16-bit tensors of the fast path, the
hi + lo planes of the split path -- and runs on whichever device the operands live on.

Two classes of inputs:

(a) EXACT.  Operands are small integers (split path: small integers in the hi planes, small integers times 2^-LO_SHIFT in the lo
    planes), bias integers, LayerScale powers of two.  check_exact asserts from |A| @ |W|^T that every output's sum of magnitudes,
    in units of the smallest term, stays below 2^24: then every partial sum in any order is exact in fp32, the result does not
    depend on tiling or k order, and the expected value is the exact one rounded ONCE to the output type.  No tolerance: bit
    equality.  Q is the exception (it carries log2(e) / 8, not a power of two): one ulp of the output type, which covers the two
    roundings fp32(v * qscale) -> T against the single one a fused multiply-convert performs.  The split planes must add up to the
    exact hh + hl + lh sum -- a lo x lo product would show.

(b) REALISTIC.  LayerNorm-like activations with outlier channels, weights on the scale of synth.make_vit_weights.  Per element

        |got - ref| <= first + C_ACC * K * 2^-24 * (|A| @ |W|^T + |bias|) * |scale| [+ g]

    first   1/2 ulp_T(ref) for a 16-bit output, 2^-24 |ref| for an fp32 one; for hi + lo planes 2^-22 |ref| (fp16; never below 2^-25,
            half the smallest fp16 subnormal: the lo plane cannot hold less) or 2^-16 |ref| (bf16), plus the dropped lo x lo term,
            2^-22 or 2^-16 times |A| @ |W|^T * |scale|
    K u     the worst-case bound of an fp32 sum of K terms in any order; C_ACC = 2 because the MFMA's internal rounding of partial
            sums is not documented.  (The split GEMMs add 3 K products; their terms hl, lh are 2^-11 of hh, so K stays the count.
            The epilogue's own fp32 operations -- bias, scale, the residual add -- are a handful of roundings against K >= 384.)
    scale   qscale for Q, LayerScale gamma for the residual updates, 1 otherwise
    g       GELU: the documented error of the approximation (gelu2: 6e-5, gelu_erfc: 4.7e-7, both from the source comments; libm erff of
            the tiled kernel: 4 fp32 ulps of max(|v|, 1) -- erff is good to an ulp of 1 + erf in [0, 2], times |v| / 2, plus the two
            multiplies), and the accumulation term grows by the GELU's Lipschitz constant 1.13.
"""
import torch

QKV, QKV_FACET, PROJ, FC1, FC2 = 0, 1, 2, 3, 4   # dtk_vit_gemm_args.role (dino_tracker_amd._lib.VIT_GEMM_*)
ROLE_NAMES = {QKV: "qkv", QKV_FACET: "qkv_facet", PROJ: "proj", FC1: "fc1", FC2: "fc2"}
# 0.125f * 1.4426950408889634f as csrc/vit.hip evaluates it (VIT_QSCALE): the fp32 literal times an exact power of two
QSCALE = 0.125 * float(torch.tensor(1.4426950408889634, dtype=torch.float32))
C_ACC = 2.0
U32 = 2.0 ** -24
G_GELU2, G_ERFC = 6e-5, 4.7e-7
GELU_LIP = 1.13
LO_SHIFT = {torch.float16: 6, torch.bfloat16: 3}      # exact class: lo planes are integers * 2^-LO_SHIFT
W_SCALE = {torch.float16: 256.0, torch.bfloat16: 1.0}  # what the model multiplies the split weight planes by (dtk_vit_layer.w_scale)


def shape(role, D):
    """(N, K) of a role at model width D."""
    return {QKV: (3 * D, D), QKV_FACET: (3 * D, D), PROJ: (D, D), FC1: (4 * D, D), FC2: (D, 4 * D)}[role]


def ulp(x, dtype):
    """ulp of `dtype` (fp16 / bf16 / fp32) at |x| (float64 tensor), subnormal range included."""
    p, emin = {torch.float16: (11, -14), torch.bfloat16: (8, -126), torch.float32: (24, -126)}[dtype]
    _, e = torch.frexp(x.abs())                       # |x| = m 2^e, m in [0.5, 1): floor(log2 |x|) = e - 1
    e = torch.where(x == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    return torch.ldexp(torch.ones_like(x), e - (p - 1))


def to_t(x64, dtype):
    """float64 -> dtype through fp32 (the route every kernel epilogue takes)."""
    return x64.float().to(dtype)


def round_once(x64, dtype):
    """An EXACT value rounded once to dtype: it must be representable in fp32, so that the fp32 stop-over rounds nothing."""
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), "exact class: a value is not representable in fp32"
    return x32.to(dtype)


def split2(x64, dtype):
    """hi = T(v), lo = T(v - hi) of an exact fp32 value (csrc/vit_split.h: split2)."""
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), "exact class: a value is not representable in fp32"
    hi = x32.to(dtype)
    return hi, (x32 - hi.float()).to(dtype)


def gelu64(v):
    return 0.5 * v * torch.special.erfc(-v * 0.7071067811865476)   # x Phi(x), no cancellation in either tail


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def _ints(g, shape, lo, hi, device):
    return torch.randint(lo, hi + 1, shape, generator=g, device=device).float()


def make_exact(role, D, rows, dtype, seed, split=False, device="cpu", fused_ln=False):
    """Integer operands of class (a).  Fast path: A in [-8, 8], W in [-4, 4].  Split path: hi planes in [-3, 3] (bf16: [-2, 2]) and lo
    planes the same integers times 2^-LO_SHIFT; the W planes are those of w_scale * W.  bias integers, gamma +- {1/2, 1, 2}."""
    N, K = shape(role, D)
    g = torch.Generator(device=device).manual_seed(seed)
    o = {"role": role, "D": D, "rows": rows, "dtype": dtype, "split": split, "w_scale": 1.0, "exact": True}
    if split:
        r = 3 if dtype == torch.float16 else 2
        sh = 2.0 ** -LO_SHIFT[dtype]
        o["A"], o["W"] = _ints(g, (rows, K), -r, r, device).to(dtype), _ints(g, (N, K), -r, r, device).to(dtype)
        o["A_lo"], o["W_lo"] = (_ints(g, (rows, K), -r, r, device) * sh).to(dtype), (_ints(g, (N, K), -r, r, device) * sh).to(dtype)
        o["w_scale"] = W_SCALE[dtype]
        o["bias"] = _ints(g, (N,), -4, 4, device)
    else:
        o["A"], o["W"] = _ints(g, (rows, K), -8, 8, device).to(dtype), _ints(g, (N, K), -4, 4, device).to(dtype)
        o["bias"] = _ints(g, (N,), -16, 16, device)
    if role in (PROJ, FC2):
        mag = torch.tensor([0.5, 1.0, 2.0], device=device)[torch.randint(0, 3, (N,), generator=g, device=device)]
        o["gamma"] = mag * (torch.randint(0, 2, (N,), generator=g, device=device).float() * 2 - 1)
        if split or fused_ln:
            o["x"] = _ints(g, (rows, N), -64, 64, device)
    if fused_ln:
        # LayerNorm parameters without cancellation in n * w + b (|n| stays below ~6 for these sums of K random products, |w| <= 1,
        # |b| >= 12): the fp32 evaluation error of the kernel's expression then stays far below the half ulp of T that check_fused_ln's
        # one-ulp bound leaves for it -- check_fused_ln asserts that margin.
        o["ln_w"] = 0.5 + 0.5 * torch.rand(N, generator=g, device=device)
        o["ln_b"] = (12.0 + 4.0 * torch.rand(N, generator=g, device=device)) * (torch.randint(0, 2, (N,), generator=g, device=device).float() * 2 - 1)
        o["ln_eps"] = 1e-6
    return o


def make_real(role, D, rows, dtype, seed, split=False, device="cpu", outlier=False, fused_ln=False):
    """Class (b): unit-Gaussian activations with three outlier channels around 30 sigma (the MLP hidden: GELU of a Gaussian), weights
    N(0, 0.04) (fc2: 0.03), bias N(0, 0.02), LayerScale 1 +- 0.1 as synth.make_vit_weights draws them; `outlier` adds what
    synth.make_outlier_vit_weights does to a block: LayerNorm gains up to 8 on the activations, LayerScale up to 3, qkv x 1.5 / fc2 x 300."""
    N, K = shape(role, D)
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)   # noqa: E731
    A = rn(rows, K)
    if role == FC2:
        A = gelu64((1.5 * A).double()).float()
    elif role == PROJ:
        A = 0.5 * A
    ch = torch.randperm(K, generator=g, device=device)[:3]
    A[:, ch] *= 30.0
    if outlier and role in (QKV, QKV_FACET, FC1):
        A = A * (1.0 + 7.0 * torch.rand(K, generator=g, device=device) ** 4)
    W = rn(N, K) * (0.03 if role == FC2 else 0.04)
    if outlier and role in (QKV, QKV_FACET):
        W[:2 * D] *= 1.5
    if outlier and role == FC2:
        W = W * 300.0
    o = {"role": role, "D": D, "rows": rows, "dtype": dtype, "split": split, "w_scale": 1.0, "exact": False, "bias": rn(N) * 0.02}
    if split:
        o["w_scale"] = W_SCALE[dtype]
        W = W * o["w_scale"]
        o["A"], o["W"] = A.to(dtype), W.to(dtype)
        o["A_lo"], o["W_lo"] = (A - o["A"].float()).to(dtype), (W - o["W"].float()).to(dtype)
    else:
        o["A"], o["W"] = A.to(dtype), W.to(dtype)
    if role in (PROJ, FC2):
        o["gamma"] = (1.0 + 0.1 * rn(N)) * ((0.5 * (1.0 + 5.0 * torch.rand(N, generator=g, device=device) ** 4)) if outlier else 1.0)
        if split or fused_ln:
            o["x"] = 3.0 * rn(rows, N)
    if fused_ln:
        o["ln_w"], o["ln_b"], o["ln_eps"] = 1.0 + 0.1 * rn(N), 0.05 * rn(N), 1e-6
    return o


# ---- the float64 reference ------------------------------------------------------------------------------------------------------------
def reference(o):
    """pre = A W^T + bias and mag = |A| @ |W|^T + |bias| in float64 (split: A = hi + lo, W = (hi + lo) / w_scale -- every product, the
    lo x lo one included).  Exact class: `mag3` leaves lo x lo out, as the kernels do."""
    A, W = o["A"].double(), o["W"].double()
    r = {}
    if o["split"]:
        Al, Wl = o["A_lo"].double(), o["W_lo"].double()
        ws = o["w_scale"]
        r["pre3"] = (A @ W.T + A @ Wl.T + Al @ W.T) / ws + o["bias"].double()          # what three products give
        r["lolo"] = (Al.abs() @ Wl.abs().T) / ws
        A, W = A + Al, (W + Wl) / ws
    r["pre"] = A @ W.T + o["bias"].double()
    r["absAW"] = A.abs() @ W.abs().T
    r["mag"] = r["absAW"] + o["bias"].double().abs()
    return r


def col_scale(o):
    """[N] float64: qscale on the Q columns, gamma on a residual update, 1 otherwise."""
    N, _ = shape(o["role"], o["D"])
    s = torch.ones(N, dtype=torch.float64, device=o["A"].device)
    if o["role"] == QKV:
        s[:o["D"]] = QSCALE
    elif o["role"] in (PROJ, FC2):
        s = o["gamma"].double()
    return s


# ---- layouts --------------------------------------------------------------------------------------------------------------------------
def qkv_scatter(C, D, S, Sp):
    """[F * S][3 D] -> q, k [F][heads][Sp][64] and vt [F][heads][64][Sp], padding zero (what the caller of the stage provides)."""
    F, heads = C.shape[0] // S, D // 64
    q = torch.zeros(F, heads, Sp, 64, dtype=C.dtype, device=C.device)
    k, vt = torch.zeros_like(q), torch.zeros(F, heads, 64, Sp, dtype=C.dtype, device=C.device)
    q[:, :, :S] = C[:, :D].reshape(F, S, heads, 64).permute(0, 2, 1, 3)
    k[:, :, :S] = C[:, D:2 * D].reshape(F, S, heads, 64).permute(0, 2, 1, 3)
    vt[:, :, :, :S] = C[:, 2 * D:].reshape(F, S, heads, 64).permute(0, 2, 3, 1)
    return q, k, vt


def qkv_gather(q, k, vt, S):
    """The inverse on the rows s < S: [F * S][3 D]."""
    F, heads = q.shape[0], q.shape[1]
    D = heads * 64
    return torch.cat([q[:, :, :S].permute(0, 2, 1, 3).reshape(F * S, D), k[:, :, :S].permute(0, 2, 1, 3).reshape(F * S, D),
                      vt[:, :, :, :S].permute(0, 3, 1, 2).reshape(F * S, D)], dim=1)


def qkv_padding_is_zero(q, k, vt, S):
    return bool((q[:, :, S:] == 0).all() and (k[:, :, S:] == 0).all() and (vt[:, :, :, S:] == 0).all())


def matrix(o, got, suffix=""):
    """A device result (dict of tensors in the stage's layouts) as one [rows][N] tensor in the OUTPUT type."""
    role = o["role"]
    if role == QKV:
        return qkv_gather(got["q" + suffix], got["k" + suffix], got["vt" + suffix], o["S"])
    if role == QKV_FACET:
        return got["out_f32"]
    if role in (PROJ, FC2) and (o["split"] or "out" not in got):
        return got["x"]
    return got["out" + suffix]


def matrix64(o, got):
    m = matrix(o, got).double()
    if o["split"] and o["role"] in (QKV, FC1):
        m = m + matrix(o, got, "_lo").double()
    return m


def _where(t):
    i = int(t.argmax())
    return divmod(i, t.shape[1])


# ---- class (a) ------------------------------------------------------------------------------------------------------------------------
def check_exact(o, got):
    """Bit equality with the exact result rounded once (module docstring, class (a)).  GELU outputs belong to class (b)."""
    role, dtype, D = o["role"], o["dtype"], o["D"]
    assert role != FC1 and o["exact"]
    r = reference(o)
    sc = col_scale(o)
    if o["split"]:
        unit = 2.0 ** -LO_SHIFT[dtype] / o["w_scale"]
        pre = r["pre3"]
        mag = r["mag"] - r["lolo"]
    else:
        unit, pre, mag = 1.0, r["pre"], r["mag"]
    if role in (PROJ, FC2):
        unit *= 0.5
        mag = mag * sc.abs()
        if "x" in o:
            mag = mag + o["x"].double().abs()
    assert float(mag.max()) / unit < 2.0 ** 24, ("exact class: sums leave fp32's integers", float(mag.max()) / unit)
    if role == QKV:
        assert qkv_padding_is_zero(got["q"], got["k"], got["vt"], o["S"]), "padding rows s >= S were written"
        if o["split"]:
            assert qkv_padding_is_zero(got["q_lo"], got["k_lo"], got["vt_lo"], o["S"]), "padding rows s >= S were written (lo)"
    if not o["split"]:
        gm = matrix(o, got)
        if role == QKV:
            want = round_once(pre[:, D:], dtype)
            bad = gm[:, D:] != want
            assert not bad.any(), ("K / V^T differ from the exact result", int(bad.sum()), _where(bad.double()))
            qref = pre[:, :D] * QSCALE
            want_q = to_t(qref, dtype).double()
            err = (gm[:, :D].double() - want_q).abs() / ulp(want_q, dtype)
            assert float(err.max()) <= 1.0, ("Q beyond one ulp of T(exact * qscale)", float(err.max()), _where(err))
        elif role == QKV_FACET:
            bad = gm.double() != pre
            assert not bad.any(), ("fp32 facet differs from the exact result", int(bad.sum()), _where(bad.double()))
        else:
            want = round_once(pre * sc, dtype)
            if "out" in got:
                bad = gm != want
                assert not bad.any(), ("delta differs from the exact result", int(bad.sum()), _where(bad.double()))
            else:
                check_fused_ln(o, got, want)
        return
    # split outputs
    if role == QKV:
        want_hi, want_lo = split2(pre[:, D:], dtype)
        assert torch.equal(want_hi.double() + want_lo.double(), pre[:, D:]), "exact class: hi + lo cannot hold the exact K / V value"
        hi, lo = matrix(o, got), matrix(o, got, "_lo")
        bad = (hi[:, D:].double() + lo[:, D:].double()) != pre[:, D:]
        assert not bad.any(), ("K / V^T planes do not add up to the exact hh + hl + lh sum", int(bad.sum()), _where(bad.double()))
        assert torch.equal(hi[:, D:], want_hi) and torch.equal(lo[:, D:], want_lo), "K / V^T planes are not split2 of the exact value"
        qref = pre[:, :D] * QSCALE
        # one ulp of a hi + lo pair: 2 x 11 (8) significant bits; fp16: never finer than 2^-24, the subnormal step of the lo plane
        pair_ulp = (2.0 ** -21 * qref.abs()).clamp(min=2.0 ** -24) if dtype == torch.float16 else (2.0 ** -15 * qref.abs()).clamp(min=2.0 ** -133)
        err = (hi[:, :D].double() + lo[:, :D].double() - qref).abs() / pair_ulp
        assert float(err.max()) <= 1.0, ("Q planes beyond one ulp of the pair", float(err.max()), _where(err))
    elif role == QKV_FACET:
        bad = got["out_f32"].double() != pre
        assert not bad.any(), ("fp32 facet differs from the exact hh + hl + lh sum", int(bad.sum()), _where(bad.double()))
    else:
        want = o["x"].double() + pre * sc
        assert torch.equal(want.float().double(), want)
        bad = got["x"].double() != want
        assert not bad.any(), ("x differs from x + gamma * (exact hh + hl + lh sum)", int(bad.sum()), _where(bad.double()))


def layernorm64(x, w, b, eps):
    x = x.double()
    mu = x.mean(dim=1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=1, keepdim=True)
    n = (x - mu) / torch.sqrt(var + eps)
    return n * w.double() + b.double(), n


def check_fused_ln(o, got, delta_want):
    """fc2 with the next block's LayerNorm in its epilogue: x bit-equal to fp32(x_in + float(delta)), ln_out within one ulp of T of the
    float64 LayerNorm of that x."""
    dtype = o["dtype"]
    x_want = o["x"] + delta_want.float()                      # one fp32 add, correctly rounded on both sides
    bad = got["x"] != x_want
    assert not bad.any(), ("fused LayerNorm: x differs from fp32(x_in + delta)", int(bad.sum()), _where(bad.double()))
    ref, n = layernorm64(x_want, o["ln_w"], o["ln_b"], o["ln_eps"])
    # the kernel evaluates (x - mean) * rstd * w + b in fp32: ~8 roundings of |n w| + |b|; the one-ulp bound leaves half an ulp for them
    margin = 8 * U32 * ((n * o["ln_w"].double()).abs() + o["ln_b"].double().abs()) / (0.5 * ulp(ref, dtype))
    assert float(margin.max()) < 0.5, ("fused LayerNorm inputs: n * w + b cancels", float(margin.max()))
    err = (got["ln_out"].double() - ref).abs() / ulp(ref, dtype)
    assert float(err.max()) <= 1.0, ("fused LayerNorm: ln_out beyond one ulp", float(err.max()), _where(err))


# ---- class (b) ------------------------------------------------------------------------------------------------------------------------
def bound(o, r, gelu_g=None):
    """(ref, bound) per element, float64 [rows][N] (module docstring, class (b)).  gelu_g: G_GELU2, G_ERFC or "erff"."""
    role, dtype, split = o["role"], o["dtype"], o["split"]
    _, K = shape(role, o["D"])
    sc = col_scale(o)
    acc = C_ACC * K * U32 * r["mag"] * sc.abs()
    ref = r["pre"] * sc
    if role == FC1:
        ref = gelu64(r["pre"])
        g = 4 * U32 * r["pre"].abs().clamp(min=1.0) if gelu_g == "erff" else float(gelu_g)
        acc = GELU_LIP * acc + g
    f32_out = role == QKV_FACET or (split and role in (PROJ, FC2))
    if role in (PROJ, FC2) and "x" in o:
        ref = o["x"].double() + ref
    if f32_out:
        first = U32 * ref.abs()
    elif split:
        first = (2.0 ** -22 * ref.abs()).clamp(min=2.0 ** -25) if dtype == torch.float16 else 2.0 ** -16 * ref.abs()
    elif role in (PROJ, FC2) and "x" in o:       # the fused LayerNorm form: the 16-bit update inside an fp32 x
        first = 0.5 * ulp(r["pre"] * sc, dtype) + U32 * ref.abs()
    else:
        first = 0.5 * ulp(ref, dtype)
    if split:
        lolo = (2.0 ** -22 if dtype == torch.float16 else 2.0 ** -16) * r["absAW"] * sc.abs()
        first = first + (GELU_LIP * lolo if role == FC1 else lolo)
    return ref, first + acc


def check_real(o, got, gelu_g=None):
    """Returns (largest |got - ref| / bound, (row, column)); raises when it exceeds 1.  QKV: also the padding."""
    r = reference(o)
    ref, b = bound(o, r, gelu_g)
    if o["role"] == QKV:
        assert qkv_padding_is_zero(got["q"], got["k"], got["vt"], o["S"]), "padding rows s >= S were written"
        if o["split"]:
            assert qkv_padding_is_zero(got["q_lo"], got["k_lo"], got["vt_lo"], o["S"]), "padding rows s >= S were written (lo)"
    g = matrix64(o, got)
    assert bool(torch.isfinite(g).all()), "non-finite output"
    ratio = (g - ref).abs() / b
    worst, at = float(ratio.max()), _where(ratio)
    assert worst <= 1.0, (f"{ROLE_NAMES[o['role']]}: |got - ref| / bound = {worst:.3f} at (row, col) {at}", float(g[at]), float(ref[at]), float(b[at]))
    return worst, at


# ---- an emulation of a correct kernel (CPU test of the test) --------------------------------------------------------------------------------
def emulate(o, lolo=False):
    """fp32 torch.matmul of the operands the device reads, the epilogue in fp32 (the GELU itself through float64, then rounded: its
    approximation is not what is emulated), rounding to T; results in the stage's layouts.  lolo: the planted defect of a FOURTH
    product in the split sum."""
    role, dtype, D = o["role"], o["dtype"], o["D"]
    bias = o["bias"].float()
    if o["split"]:
        Ah, Al, Wh, Wl = o["A"].float(), o["A_lo"].float(), o["W"].float(), o["W_lo"].float()
        acc = Ah @ Wl.T + Al @ Wh.T
        if lolo:
            acc = acc + Al @ Wl.T
        acc = acc + Ah @ Wh.T
        v = acc * (1.0 / o["w_scale"]) + bias
    else:
        v = o["A"].float() @ o["W"].float().T + bias
    sc = col_scale(o).float()
    got = {}

    def planes(x32):
        hi = x32.to(dtype)
        return hi, (x32 - hi.float()).to(dtype)

    if role == QKV:
        u = v * sc
        if o["split"]:
            hi, lo = planes(u)
            got["q"], got["k"], got["vt"] = qkv_scatter(hi, D, o["S"], o["Sp"])
            got["q_lo"], got["k_lo"], got["vt_lo"] = qkv_scatter(lo, D, o["S"], o["Sp"])
        else:
            got["q"], got["k"], got["vt"] = qkv_scatter(u.to(dtype), D, o["S"], o["Sp"])
    elif role == QKV_FACET:
        got["out_f32"] = v
    elif role == FC1:
        u = gelu64(v.double()).float()
        if o["split"]:
            got["out"], got["out_lo"] = planes(u)
        else:
            got["out"] = u.to(dtype)
    elif o["split"]:
        got["x"] = o["x"] + sc * v
    else:
        d = (sc * v).to(dtype)
        if "ln_w" in o:   # fc2 with the next block's LayerNorm: layernorm_kernel's expressions in fp32
            x = o["x"] + d.float()
            mu = x.mean(dim=1, keepdim=True)
            rstd = torch.rsqrt(((x - mu) ** 2).mean(dim=1, keepdim=True) + o["ln_eps"])
            got["x"], got["ln_out"] = x, ((x - mu) * rstd * o["ln_w"] + o["ln_b"]).to(dtype)
        else:
            got["out"] = d
    return got


# ---- row counts from the kernels' grids ---------------------------------------------------------------------------------------------------
WS_ROWS, WS_COLS = 32, 256


def ws_grid(N, rows):
    """(chunks launched, token tiles per chunk, tiles of the last chunk): csrc/vit_gemm_ws.h gemm_ws_grid."""
    colwg = -(-N // WS_COLS)
    chunks = max(256 // colwg, 1)
    tiles = -(-rows // WS_ROWS)
    tpc = -(-tiles // chunks)
    nch = -(-tiles // tpc)
    return nch, tpc, tiles - (nch - 1) * tpc


def ws_rows_for(N, tpc_min, tpc_max, step=1):
    """The smallest row count, a multiple of `step` with a ragged last tile (17 rows where step leaves the choice), whose grid has tpc_min <= tiles per chunk <= tpc_max, more
    than one chunk and a last chunk shorter than the others."""
    for m in range(1, 1 << 20):
        rows = m * step
        nch, tpc, last = ws_grid(N, rows)
        if tpc > tpc_max:
            break
        if tpc >= tpc_min and nch > 1 and last < tpc and (rows % WS_ROWS == 17 if step == 1 else rows % WS_ROWS):
            return rows
    raise AssertionError((N, tpc_min, tpc_max, step))
