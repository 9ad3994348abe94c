"""GPU: the RAFT stages around the convolutions, each alone against the float64 restatement of tests/raft_ref.py (instance norm,
correlation pyramid, lookup, convex upsampling).  Bounds are derived per test from fp32 rounding of the stage's own arithmetic."""
import pytest
import torch
import torch.nn.functional as F

import raft_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -24


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().to(DEV)


def nchw(t):
    return t.permute(0, 3, 1, 2).double().cpu()


# ---- instance norm
@pytest.mark.parametrize("shape", [(2, 64, 13, 17), (2, 96, 1, 19), (1, 128, 40, 33)])
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
def test_instance_norm(shape, relu, res):
    """13 x 17 x 64, a one-row image and a size with several pixel chunks (1320 pixels: 3 chunks); one channel is constant (its
    variance is 0: the output is 0 / sqrt(eps) = 0) and one has a large offset (mean 100: the two-pass variance must not cancel).
    Bound: the statistics are sums of hw fp32 terms (relative hw 2^-24 on the mean and the variance, the mean's error scaled
    by 1 / std), then three roundings: (4 + hw) 2^-23 (1 + |y|) + hw 2^-24 |mean| / std."""
    from dino_tracker_amd import raft
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g)
    x[:, 1] = 3.25
    x[:, 2] += 100.0
    x = x.float().double()
    r = torch.rand(*shape, generator=g).float().double() if res else None
    y = R.instance_norm(x)
    ref = torch.relu(y) if relu else y
    if res:
        ref = torch.relu(r + ref)
    got = nchw(raft.instance_norm(nhwc(x), relu=relu, res=nhwc(r) if res else None))
    hw = shape[2] * shape[3]
    mean = x.mean(dim=(2, 3), keepdim=True).abs()
    std = torch.sqrt(x.var(dim=(2, 3), unbiased=False, keepdim=True) + 1e-5)
    bd = (4 + hw) * 2 * EPS32 * (1 + y.abs()) + hw * EPS32 * mean / std
    worst = ((got - ref).abs() / bd).max().item()
    print(f"instance norm {shape} relu={relu} res={res}: max err {(got - ref).abs().max().item():.3e}, err / bound {worst:.3f}")
    assert worst <= 1.0
    if not res:
        assert not got[:, 1].any()      # the constant channel: exactly zero


def test_instance_norm_is_deterministic():
    from dino_tracker_amd import raft
    x = torch.randn(2, 40, 33, 128, generator=torch.Generator().manual_seed(1)).to(DEV)
    a, b = raft.instance_norm(x, relu=True), raft.instance_norm(x, relu=True)
    assert torch.equal(a, b)


# ---- correlation pyramid
@pytest.mark.parametrize("h,w", [(16, 17), (17, 16)])
@pytest.mark.parametrize("mode", ["split", "fp16"])
def test_corr_pyramid(h, w, mode):
    """Level 0 against the float64 inner products (of the fp16-rounded features in fp16 mode); levels 1 .. 3 drop the odd column /
    row.  Bound per element of level 0: 2 C 2^-24 sum|a b| / 16 accumulation + the split representation (da |b| + |a| db + 2^-22 |a b|
    summed, / 16, with da = max(2^-22 |a|, 2^-25) as include/dtk.h states it);
    every pooling adds three fp32 additions and a scaling: 4 x 2^-24 of the mean of the |values| it averages, bounded by the level-0 maximum."""
    from dino_tracker_amd import raft
    g = torch.Generator().manual_seed(h * 100 + w)
    f1, f2 = (torch.randn(2, 256, h, w, generator=g).float().double() for _ in range(2))
    got = raft.corr_pyramid(nhwc(f1), nhwc(f2), mode)[:4]
    ref = R.corr_pyramid(f1, f2, R.fp16_round if mode == "fp16" else None)
    a, b = (f1.flatten(2), f2.flatten(2)) if mode == "split" else (R.fp16_round(f1.flatten(2)), R.fp16_round(f2.flatten(2)))
    dot = lambda u, v: torch.einsum("nci,ncj->nij", u, v) / 16   # noqa: E731
    mag = dot(a.abs(), b.abs())
    bd0 = 2 * 256 * EPS32 * mag + 2 * EPS32 * ref[0].view(2, h * w, h * w).abs()
    if mode == "split":
        d = lambda u: torch.maximum(2.0 ** -22 * u.abs(), torch.full_like(u, 2.0 ** -25))   # noqa: E731
        bd0 = bd0 + dot(d(a), b.abs()) + dot(a.abs(), d(b)) + 2.0 ** -22 * mag
    e0 = (got[0].double().cpu().view(2, h * w, h * w) - ref[0].view(2, h * w, h * w)).abs()
    print(f"corr {h}x{w} {mode}: level 0 max err {e0.max().item():.3e}, err / bound {(e0 / bd0).max().item():.3f}")
    assert (e0 / bd0).max().item() <= 1.0
    hl, wl = h, w
    for l in range(1, 4):
        hl, wl = hl // 2, wl // 2
        assert got[l].shape == (2, h * w, hl, wl)
        e = (got[l].double().cpu().reshape(-1) - ref[l].reshape(-1)).abs().max().item()
        bd = bd0.max().item() + 4 * l * EPS32 * ref[0].abs().max().item()
        print(f"corr {h}x{w} {mode}: level {l} max err {e:.3e} (bound {bd:.3e})")
        assert e <= bd


def test_corr_pyramid_minimum_size():
    from dino_tracker_amd import raft
    f = torch.zeros(1, 15, 16, 256, device=DEV)
    with pytest.raises(ValueError, match="16 x 16"):
        raft.corr_pyramid(f, f)


# ---- lookup
H_, W_ = 16, 19


@pytest.fixture(scope="module")
def pyramid():
    from dino_tracker_amd import raft
    g = torch.Generator().manual_seed(5)
    f1, f2 = (torch.randn(1, 256, H_, W_, generator=g).float() for _ in range(2))
    levels = raft.corr_pyramid(nhwc(f1), nhwc(f2))
    ref_levels = [lv.double().cpu().reshape(H_ * W_, 1, lv.shape[2], lv.shape[3]) for lv in levels[:4]]   # the device's own maps
    return levels[4], ref_levels


def planted_flow(kind):
    """flow [1, 2, H_, W_]: coordinates = grid + flow land where the case wants them"""
    grid = R.coords_grid(1, H_, W_, torch.float64)
    target = grid.clone()
    if kind == "integer":
        target[:, 0] = (grid[:, 0] + 3) % W_
        target[:, 1] = (grid[:, 1] + 5) % H_
    elif kind == "half":
        target = target + 0.5
    elif kind == "fraction":
        target[:, 0] += 0.3125
        target[:, 1] -= 1.8125
    elif kind == "negative":
        target[:, 0] = -2.25 - grid[:, 0] / 8
        target[:, 1] = -0.75
    elif kind == "outside":
        target[:, 0] = W_ + 45.5           # more than the radius beyond every level's map (level 3: 8.1 > 2 + 5)
        target[:, 1] = -60.0
    elif kind == "last_cell":
        target[:, 0] = 8.0 * (W_ // 8 - 1)   # exactly the last cell of level 3 (2 x 2): (8, 8) / 8 = (1, 1)
        target[:, 1] = 8.0 * (H_ // 8 - 1)
    return (target - grid).float().double(), grid


@pytest.mark.parametrize("kind", ["integer", "half", "fraction", "negative", "outside", "last_cell"])
def test_lookup_planted(pyramid, kind):
    """The reads are bilinear on the SAME fp32 maps (the device's own pyramid), so the only error is the fp32 evaluation of four
    products and three additions of values <= max|map|: 8 x 2^-24 max|map|.  Integer coordinates read single cells exactly."""
    from dino_tracker_amd import raft
    buf, ref_levels = pyramid
    flow, grid = planted_flow(kind)
    got = nchw(raft.lookup(buf, nhwc(flow)))
    ref = R.lookup(ref_levels, grid + flow)
    top = max(lv.abs().max().item() for lv in ref_levels)
    err = (got - ref).abs().max().item()
    print(f"lookup {kind}: max err {err:.3e} (bound {8 * EPS32 * top:.3e})")
    assert err <= 8 * EPS32 * top
    if kind == "outside":
        assert not got.any()
    if kind == "integer":
        assert torch.equal(got[:, :81], ref[:, :81])
    if kind == "last_cell":      # level 3, window centre (a, b) = (4, 4): the map's last cell itself
        lv3 = ref_levels[3]
        assert torch.equal(got[0, 3 * 81 + 40].reshape(-1), lv3[:, 0, -1, -1])


def test_lookup_channel_order():
    """A level-0 map with a single non-zero cell at (x, y) = (6, 3) for every source cell, coordinates (4, 4) everywhere: the
    window reads x + a - 4 = 6 at a = 6 and y + b - 4 = 3 at b = 3, so exactly channel 9 a + b = 57 is non-zero (the transposed
    order would light channel 9 x 3 + 6 = 33)."""
    from dino_tracker_amd import _lib, raft
    h, w = 16, 16
    n = int(_lib.lib().dtk_raft_pyramid_floats(1, h, w))
    buf = torch.zeros(n, device=DEV)
    buf[:h * w * h * w].view(h * w, h, w)[:, 3, 6] = 2.0
    grid = R.coords_grid(1, h, w, torch.float64)
    flow = torch.full((1, 2, h, w), 4.0, dtype=torch.float64) - grid
    got = nchw(raft.lookup(buf, nhwc(flow)))
    lit = got[0].flatten(1).abs().sum(1).nonzero().flatten().tolist()
    assert lit == [57], lit
    assert torch.equal(got[0, 57], torch.full((h, w), 2.0, dtype=torch.float64))


def test_lookup_writes_its_slice_only(pyramid):
    from dino_tracker_amd import raft
    buf, _ = pyramid
    flow, _ = planted_flow("fraction")
    wide = torch.full((1, H_, W_, 330), 7.0, device=DEV)
    raft.lookup(buf, nhwc(flow), out=wide[..., 3:327])
    assert bool((wide[..., :3] == 7.0).all() and (wide[..., 327:] == 7.0).all())
    assert torch.equal(wide[..., 3:327], raft.lookup(buf, nhwc(flow)))


# ---- convex upsampling
@pytest.mark.parametrize("kind", ["random", "dominant", "constant"])
def test_upsample(kind):
    """random masks; a mask with one dominant tap (+60: the softmax is that tap to 1e-26, the output 8 x the neighbour's flow); a
    constant mask (the 3 x 3 mean with zero padding).  Bound: the softmax weights carry the documented 4.8e-7 relative exp error
    and the sums nine fp32 terms: (2 x 4.8e-7 + 12 x 2^-24) x 8 max|flow|."""
    from dino_tracker_amd import raft
    h, w = 5, 7
    g = torch.Generator().manual_seed(9)
    flow = (torch.randn(2, 2, h, w, generator=g) * 3).float().double()
    if kind == "random":
        mask = torch.randn(2, 576, h, w, generator=g) * 2
    elif kind == "dominant":
        mask = torch.randn(2, 576, h, w, generator=g)
        mask[:, 64 * 2:64 * 3] += 60.0       # tap k = 2: (y - 1, x + 1)
    else:
        mask = torch.full((2, 576, h, w), 1.5)
    mask = mask.float().double()
    wide = torch.zeros(2, h, w, 6, device=DEV)
    wide[..., 3:5] = nhwc(flow)              # the flow as a slice at an odd offset
    got = raft.upsample(wide[..., 3:5], nhwc(mask)).double().cpu()
    ref = R.upsample(flow, mask)
    bd = (2 * 4.8e-7 + 12 * EPS32) * 8 * flow.abs().max().item()
    err = (got - ref).abs().max().item()
    print(f"upsample {kind}: max err {err:.3e} (bound {bd:.3e})")
    assert got.shape == (2, 2, 8 * h, 8 * w) and err <= bd
    if kind == "dominant":
        shifted = F.pad(8 * flow, (0, 1, 1, 0))[:, :, :h, 1:]     # flow(y - 1, x + 1), zero outside
        assert (got - shifted.repeat_interleave(8, 2).repeat_interleave(8, 3)).abs().max().item() <= bd
