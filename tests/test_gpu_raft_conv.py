"""GPU: the RAFT convolution kernel (dtk_raft_conv) alone against float64, for every (kernel, stride, Cin, Cout) the network uses,
N = 2 at 9 x 11 and 16 x 17 (odd sizes, stride-2 flooring, a ragged last tile, fewer pixels than a tile), both operand modes.

Two classes, as in tests/vit_gemm_ref.py:
* integer operands whose partial sums are exact in fp32 (|x| <= 8, |w| <= 4, K <= 3456: |sum| < 2^17): BIT-equal;
* realistic operands, per element
      |out - ref| <= 2 K 2^-24 (|x| (*) |w| + |b|)                      accumulation: K fp32 additions in any order, twice over
                   + |w| (*) dx + dw (*) |x| + 2^-22 |x| (*) |w|          split representation (include/dtk.h): dx = max(2^-22 |x|, 2^-25),
                                                                         dw = max(2^-22 |w|, 2^-25 / wscale); the dropped lo.lo term
                   + 4.8e-7 for sigmoid / tanh (the documented bound; both are 1-Lipschitz) + 2^-23 |ref|   the result's own rounding
  where (*) is the convolution of the absolute values.  In fp16 mode the reference is the float64 convolution of the operands
  rounded to fp16, whose products are exact: the representation terms vanish.
The output is a channel slice of a wider tensor with guard values around it: the neighbouring channels and the floats behind
the buffer must stay untouched.  The 9 x 11 case uses slices at channel offset 3 (element-wise loads and stores), the 16 x 17 case
offset 4 (16-byte loads and stores)."""
import pytest
import torch
import torch.nn.functional as F

from dino_tracker_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 12345.0
SIZES = ((9, 11, 3), (16, 17, 4))      # H, W, channel offset of the slices
# (kh, kw, stride, cin, cout) -- the network's combinations
COMBOS = [(7, 7, 2, 3, 64), (3, 3, 1, 64, 64), (3, 3, 2, 64, 96), (1, 1, 2, 64, 96), (3, 3, 1, 96, 96), (3, 3, 2, 96, 128),
          (1, 1, 2, 96, 128), (3, 3, 1, 128, 128), (1, 1, 1, 128, 256), (1, 1, 1, 128, 128), (1, 1, 1, 324, 256), (3, 3, 1, 256, 192),
          (7, 7, 1, 2, 128), (3, 3, 1, 128, 64), (3, 3, 1, 256, 126), (1, 5, 1, 384, 128), (5, 1, 1, 384, 128), (3, 3, 1, 128, 256),
          (3, 3, 1, 256, 2), (1, 1, 1, 256, 576)]
ACTS = {"none": _lib.RAFT_ACT_NONE, "relu": _lib.RAFT_ACT_RELU, "sigmoid": _lib.RAFT_ACT_SIGMOID, "tanh": _lib.RAFT_ACT_TANH}
ACT_ERR = 4.8e-7


def activate(t, act):
    return {"none": lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act](t)


def fp16r(t):
    return t.to(torch.float16).to(t.dtype)


def operands(kh, kw, cin, cout, H, W, integer, seed):
    g = torch.Generator().manual_seed(seed)
    if integer:
        x = torch.randint(-8, 9, (2, cin, H, W), generator=g).double()
        w = torch.randint(-4, 5, (cout, cin, kh, kw), generator=g).double()
        b = torch.randint(-16, 17, (cout,), generator=g).double()
    else:
        x = torch.randn(2, cin, H, W, generator=g).float().double()
        w = (torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cout * kh * kw)) ** 0.5).float().double()
        b = (torch.rand(cout, generator=g) - 0.5).float().double()
    return x, w, b


def sliced(t_nchw, off, extra=5):
    """an NHWC device tensor wider than the data, guard-filled, with the data at channels off .. off + C; returns (whole, view)"""
    n, c, h, w = t_nchw.shape
    whole = torch.full((n, h, w, c + off + extra), GUARD, dtype=torch.float32, device=DEV)
    view = whole[..., off:off + c]
    view.copy_(t_nchw.permute(0, 2, 3, 1).float())
    return whole, view


def device_conv(x, w, b, stride, pad, mode, act, off, x2_split=None, res=None, res_relu=False, mul=None, gate=None, h_old=None):
    """runs dtk_raft_conv with the output in a guarded slice; returns the result [N, Cout, Ho, Wo] float64 and the guard report"""
    from dino_tracker_amd import raft
    pc = raft.PackedConv(w.float(), b.float(), stride, pad[0], pad[1], DEV)
    if x2_split is None:
        _, xv = sliced(x, off)
        x2v = None
    else:
        _, xv = sliced(x[:, :x2_split], off)
        _, x2v = sliced(x[:, x2_split:], off)
    cout, kh, kw = w.shape[0], w.shape[2], w.shape[3]
    Ho, Wo = (x.shape[2] + 2 * pad[0] - kh) // stride + 1, (x.shape[3] + 2 * pad[1] - kw) // stride + 1
    n_out = 2 * Ho * Wo * (cout + off + 5)
    flat = torch.full((n_out + 64,), GUARD, dtype=torch.float32, device=DEV)
    whole = flat[:n_out].view(2, Ho, Wo, cout + off + 5)
    out = whole[..., off:off + cout]
    if h_old is not None:
        out.copy_(h_old.permute(0, 2, 3, 1).float())
    aux = {k: (sliced(v, off)[1] if v is not None else None) for k, v in (("res", res), ("mul", mul), ("gate", gate))}
    raft.conv2d(xv, pc, out, mode, ACTS[act], x2=x2v, res=aux["res"], res_relu=res_relu, mul=aux["mul"], gate=aux["gate"])
    torch.cuda.synchronize()
    untouched = bool((whole[..., :off] == GUARD).all() and (whole[..., off + cout:] == GUARD).all() and (flat[n_out:] == GUARD).all())
    return out.permute(0, 3, 1, 2).double().cpu(), untouched, pc.scale


def bound(x, w, b, stride, pad, mode, act, ref, wscale):
    K = w.shape[1] * w.shape[2] * w.shape[3]
    ax, aw = x.abs(), w.abs()
    conv = lambda a, c: F.conv2d(a, c, None, stride, pad)   # noqa: E731
    bd = 2 * K * 2.0 ** -24 * (conv(ax, aw) + b.abs().view(1, -1, 1, 1))
    if mode == "split":
        dx = torch.maximum(2.0 ** -22 * ax, torch.full_like(ax, 2.0 ** -25))
        dw = torch.maximum(2.0 ** -22 * aw, torch.full_like(aw, 2.0 ** -25 / wscale))
        bd = bd + conv(dx, aw) + conv(ax, dw) + 2.0 ** -22 * conv(ax, aw)
    if act in ("sigmoid", "tanh"):
        bd = bd + ACT_ERR
    return bd + 2.0 ** -23 * ref.abs()


@pytest.mark.parametrize("kh,kw,stride,cin,cout", COMBOS)
def test_conv_against_float64(kh, kw, stride, cin, cout):
    pad = (kh // 2, kw // 2)
    act = "relu" if cout % 3 else "none"
    for H, W, off in SIZES:
        for integer in (True, False):
            x, w, b = operands(kh, kw, cin, cout, H, W, integer, seed=kh * 1000 + cin + cout + H)
            for mode in ("split", "fp16"):
                xr, wr = (x, w) if mode == "split" or integer else (fp16r(x), fp16r(w))
                ref = activate(F.conv2d(xr, wr, b, stride, pad), act)
                got, untouched, wscale = device_conv(x, w, b, stride, pad, mode, act, off)
                assert untouched, (H, W, mode, "the kernel wrote outside its channel slice")
                assert got.shape == ref.shape
                if integer:
                    assert torch.equal(got, ref), (H, W, mode, (got - ref).abs().max().item())
                else:
                    bd = bound(xr, wr, b, stride, pad, mode, act, ref, wscale)
                    worst = ((got - ref).abs() / bd).max().item()
                    print(f"conv {kh}x{kw} s{stride} {cin}->{cout} {H}x{W} {mode}: max err {(got - ref).abs().max().item():.3e}, "
                          f"worst err / bound {worst:.3f}")
                    assert worst <= 1.0, (H, W, mode, worst)


@pytest.mark.parametrize("mode", ["split", "fp16"])
@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
def test_conv_epilogues(mode, act):
    """The GRU shapes: two input sources (128 | 256 channels), sigmoid x mul (r h), tanh + gate in place ((1 - z) h + z q), and a
    residual add with and without the ReLU; the activations within their documented 4.8e-7."""
    g = torch.Generator().manual_seed(7)
    H, W, off = 9, 11, 4
    x, w, b = operands(1, 5, 384, 128, H, W, False, seed=11)
    x = x * 0.5
    aux = torch.rand(2, 128, H, W, generator=g).float().double()
    hold = (torch.rand(2, 128, H, W, generator=g) * 2 - 1).float().double()
    xr, wr = (x, w) if mode == "split" else (fp16r(x), fp16r(w))
    pre = F.conv2d(xr, wr, b, 1, (0, 2))
    a = activate(pre, act)
    for kind in ("mul", "gate", "res", "res_relu"):
        kw = {}
        if kind == "mul":
            ref, kw, scale = a * aux, dict(mul=aux), aux
        elif kind == "gate":
            ref, kw, scale = (1 - aux) * hold + aux * a, dict(gate=aux, h_old=hold), aux
        else:
            ref = a + hold
            ref, kw, scale = (torch.relu(ref) if kind == "res_relu" else ref), dict(res=hold, res_relu=kind == "res_relu"), 1.0
        got, untouched, wscale = device_conv(x, w, b, 1, (0, 2), mode, act, off, x2_split=128, **kw)
        assert untouched, kind
        # the epilogue's own operations: a few fp32 roundings of values <= 2 on top of the convolution's bound scaled by the factor
        bd = bound(xr, wr, b, 1, (0, 2), mode, act, a, wscale) * scale + 4 * 2.0 ** -23
        worst = ((got - ref).abs() / bd).max().item()
        print(f"epilogue {kind} {act} {mode}: max err {(got - ref).abs().max().item():.3e}, worst err / bound {worst:.3f}")
        assert worst <= 1.0, (kind, worst)


@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
def test_activation_accuracy(act):
    """An identity 1 x 1 convolution on fp16-exact inputs k / 64, |k| <= 768, gives the pre-activation exactly, so the whole error
    is the activation's: within the documented 4.8e-7 absolute over [-12, 12], in both modes."""
    from dino_tracker_amd import raft
    pc = raft.PackedConv(torch.eye(64).view(64, 64, 1, 1), torch.zeros(64), 1, 0, 0, DEV)
    x = (torch.arange(-768, 768, dtype=torch.float64) / 64).view(1, 24, 1, 64)     # NHWC: 24 pixels of 64 channels
    for mode in ("split", "fp16"):
        out = torch.empty(1, 24, 1, 64, device=DEV)
        raft.conv2d(x.float().to(DEV), pc, out, mode, ACTS[act])
        err = (out.double().cpu() - activate(x, act)).abs().max().item()
        print(f"{act} {mode}: max abs err {err:.3e}")
        assert err <= ACT_ERR


def test_flow_update_in_place():
    """flow += delta: the residual is the output slice itself (two channels at an odd offset of a 384-wide tensor)."""
    H, W = 16, 17
    x, w, b = operands(3, 3, 256, 2, H, W, True, seed=3)
    from dino_tracker_amd import raft
    pc = raft.PackedConv(w.float(), b.float(), 1, 1, 1, DEV)
    g = torch.Generator().manual_seed(4)
    hx = torch.randint(-5, 6, (2, H, W, 384), generator=g).float().to(DEV)
    before = hx.clone()
    xin = x.permute(0, 2, 3, 1).float().contiguous().to(DEV)
    flow = hx[..., 382:384]
    raft.conv2d(xin, pc, flow, "split", _lib.RAFT_ACT_NONE, res=flow)
    ref = F.conv2d(x, w, b, 1, 1).permute(0, 2, 3, 1) + before[..., 382:].double().cpu()
    assert torch.equal(hx[..., 382:].double().cpu(), ref)
    assert torch.equal(hx[..., :382], before[..., :382])


def test_conv_refusals():
    from dino_tracker_amd import raft
    pc = raft.PackedConv(torch.zeros(4, 8, 3, 3), torch.zeros(4), 1, 1, 1, DEV)
    x = torch.zeros(1, 9, 9, 8, device=DEV)
    out = torch.full((1, 9, 9, 4), GUARD, device=DEV)
    with pytest.raises(RuntimeError, match="second input"):
        raft.conv2d(x[..., :4], pc, out, x2=x[..., 4:])          # a split that is no multiple of 32
    with pytest.raises(RuntimeError, match="activation"):
        raft.conv2d(x, pc, out, act=9)
    with pytest.raises(RuntimeError, match="not on a GPU"):
        raft.conv2d(x.cpu(), pc, out)
    assert bool((out == GUARD).all())
