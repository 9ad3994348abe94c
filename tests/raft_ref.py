"""RAFT-large (torchvision's raft_large) restated in plain torch from the published definition, dtype-generic (float64 is the
yardstick, float32 gives the yardstick's own error).  No torchvision.  The state dict uses torchvision's key names.

`rnd` rounds the operands of every convolution and of the correlation (activations and weights): `fp16_round` emulates the device's
fp16 operand mode in float64.  For that emulation pass a state dict whose BatchNorms are already folded (raft.fold_batchnorm):
the device rounds the FOLDED weights.

`defect` plants one mistake at a time (DEFECTS); tests/test_raft_reference.py checks that the comparison rejects each.
"""
import math

import torch
import torch.nn.functional as F

DEFECTS = ("offsets_yx", "no_level_scale", "no_corr_scale", "border_lookup", "softmax_axis", "unfolded_bn", "swap_z")
BN_EPS = 1e-5


def fp16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float16).to(t.dtype)


def conv(x, sd, name, stride=1, padding=0, rnd=None):
    w, b = sd[name + ".weight"].to(x.dtype), sd[name + ".bias"].to(x.dtype)
    if rnd is not None:
        x, w = rnd(x), rnd(w)
    return F.conv2d(x, w, b, stride, padding)


def instance_norm(x, eps=1e-5):
    mean = x.mean(dim=(2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(2, 3), keepdim=True)
    return (x - mean) / torch.sqrt(var + eps)


def _batch_norm(x, sd, name):
    if name + ".running_mean" not in sd:    # a folded state dict
        return x
    g, b, m, v = (sd[f"{name}.{f}"].to(x.dtype).view(1, -1, 1, 1) for f in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / torch.sqrt(v + BN_EPS) * g + b


def encoder(x, sd, prefix, norm, rnd=None, defect=None):
    def cna(x, name, stride, k, act=True):
        y = conv(x, sd, name + ".0", stride, k // 2, rnd)
        if norm == "instance":
            y = instance_norm(y)
        elif defect != "unfolded_bn":
            y = _batch_norm(y, sd, name + ".1")
        return F.relu(y) if act else y

    x = cna(x, prefix + ".convnormrelu", 2, 7)
    for layer, stride in ((1, 1), (2, 2), (3, 2)):
        for blk in range(2):
            s = stride if blk == 0 else 1
            p = f"{prefix}.layer{layer}.{blk}"
            y = cna(cna(x, p + ".convnormrelu1", s, 3), p + ".convnormrelu2", 1, 3)
            if s != 1:
                x = cna(x, p + ".downsample", s, 1, act=False)
            x = F.relu(x + y)
    return conv(x, sd, prefix + ".conv", 1, 0, rnd)


def corr_pyramid(f1, f2, rnd=None, defect=None):
    """f1, f2 [N, C, h, w] -> 4 levels [N h w, 1, h_l, w_l]."""
    N, C, h, w = f1.shape
    if h < 16 or w < 16:
        raise ValueError(f"the feature map must be at least 16 x 16 (images of 128 x 128), got {h} x {w}")
    a, b = f1.flatten(2), f2.flatten(2)
    if rnd is not None:
        a, b = rnd(a), rnd(b)
    corr = torch.einsum("nci,ncj->nij", a, b)
    if defect != "no_corr_scale":
        corr = corr / math.sqrt(C)
    corr = corr.reshape(N * h * w, 1, h, w)
    pyr = [corr]
    for _ in range(3):
        corr = F.avg_pool2d(corr, 2, 2)
        pyr.append(corr)
    return pyr


def bilinear_zero(img, pts, border=False):
    """img [B, 1, H, W]; pts [B, ..., 2] (x, y) in pixels, align_corners=True; zeros outside (or border clamping)."""
    B, _, H, W = img.shape
    x, y = pts[..., 0], pts[..., 1]
    if border:
        x, y = x.clamp(0, W - 1), y.clamp(0, H - 1)
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    flat = img.reshape(B, H * W)

    def at(xi, yi):
        ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
        idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long().reshape(B, -1)
        return flat.gather(1, idx).reshape(x.shape) * ok.to(img.dtype)

    return ((1 - fx) * (1 - fy) * at(x0, y0) + fx * (1 - fy) * at(x0 + 1, y0) + (1 - fx) * fy * at(x0, y0 + 1)
            + fx * fy * at(x0 + 1, y0 + 1))


def lookup(pyr, coords, defect=None):
    """coords [N, 2, h, w] (x, y) -> [N, 324, h, w]; channel 81 l + 9 a + b reads level l at (x / 2^l + a - 4, y / 2^l + b - 4)."""
    N, _, h, w = coords.shape
    c = coords.permute(0, 2, 3, 1).reshape(N * h * w, 1, 1, 2)
    d = torch.arange(-4, 5, dtype=coords.dtype)
    da, db = torch.meshgrid(d, d, indexing="ij")       # [a][b]: a is the slow index
    delta = torch.stack((db, da) if defect == "offsets_yx" else (da, db), dim=-1).view(1, 9, 9, 2)
    out = []
    for l, corr in enumerate(pyr):
        cl = c if defect == "no_level_scale" else c / 2 ** l
        out.append(bilinear_zero(corr, cl + delta, border=defect == "border_lookup").reshape(N, h, w, 81))
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2)


def update_block(sd, h, context, corr_feat, flow, rnd=None, defect=None):
    m, g, u = "update_block.motion_encoder", "update_block.recurrent_block", "update_block.flow_head"
    cor = F.relu(conv(corr_feat, sd, f"{m}.convcorr1.0", 1, 0, rnd))
    cor = F.relu(conv(cor, sd, f"{m}.convcorr2.0", 1, 1, rnd))
    flo = F.relu(conv(flow, sd, f"{m}.convflow1.0", 1, 3, rnd))
    flo = F.relu(conv(flo, sd, f"{m}.convflow2.0", 1, 1, rnd))
    mo = F.relu(conv(torch.cat((cor, flo), 1), sd, f"{m}.conv.0", 1, 1, rnd))
    x = torch.cat((context, mo, flow), 1)
    for gru, pad in (("convgru1", (0, 2)), ("convgru2", (2, 0))):
        hx = torch.cat((h, x), 1)
        z = torch.sigmoid(conv(hx, sd, f"{g}.{gru}.convz", 1, pad, rnd))
        r = torch.sigmoid(conv(hx, sd, f"{g}.{gru}.convr", 1, pad, rnd))
        q = torch.tanh(conv(torch.cat((r * h, x), 1), sd, f"{g}.{gru}.convq", 1, pad, rnd))
        h = z * h + (1 - z) * q if defect == "swap_z" else (1 - z) * h + z * q
    delta = conv(F.relu(conv(h, sd, f"{u}.conv1", 1, 1, rnd)), sd, f"{u}.conv2", 1, 1, rnd)
    return h, delta


def mask_predictor(sd, h, rnd=None):
    return 0.25 * conv(F.relu(conv(h, sd, "mask_predictor.convrelu.0", 1, 1, rnd)), sd, "mask_predictor.conv", 1, 0, rnd)


def upsample(flow, mask, defect=None):
    """flow [N, 2, h, w], mask [N, 576, h, w] -> [N, 2, 8 h, 8 w]."""
    N, _, h, w = flow.shape
    mask = mask.view(N, 1, 9, 8, 8, h, w)
    mask = torch.softmax(mask, dim=3 if defect == "softmax_axis" else 2)
    up = F.unfold(8 * flow, kernel_size=3, padding=1).view(N, 2, 9, 1, 1, h, w)
    up = (mask * up).sum(dim=2)
    return up.permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * h, 8 * w)


def coords_grid(N, h, w, dtype):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
    return torch.stack((xs, ys), 0)[None].repeat(N, 1, 1, 1)


@torch.no_grad()
def raft_forward(sd, image1, image2, num_flow_updates=24, dtype=torch.float64, rnd=None, defect=None, return_at=None):
    """image1, image2 [N, 3, H, W] in [-1, 1] -> the last flow prediction [N, 2, H, W] in `dtype`.  return_at: update counts k ->
    a dict {k: the prediction after k updates} instead (what num_flow_updates = k returns), from one pass."""
    image1, image2 = image1.to(dtype), image2.to(dtype)
    N, _, H, W = image1.shape
    if H % 8 or W % 8:
        raise ValueError("image sizes must be divisible by 8")
    fmaps = encoder(torch.cat((image1, image2)), sd, "feature_encoder", "instance", rnd, defect)
    pyr = corr_pyramid(fmaps[:N], fmaps[N:], rnd, defect)
    ctx = encoder(image1, sd, "context_encoder", "batch", rnd, defect)
    h, context = torch.tanh(ctx[:, :128]), F.relu(ctx[:, 128:])
    coords0 = coords_grid(N, H // 8, W // 8, dtype)
    coords1 = coords0.clone()
    preds = {}
    for it in range(1, num_flow_updates + 1):
        corr_feat = lookup(pyr, coords1, defect)
        h, delta = update_block(sd, h, context, corr_feat, coords1 - coords0, rnd, defect)
        coords1 = coords1 + delta
        if return_at is not None and it in return_at:
            preds[it] = upsample(coords1 - coords0, mask_predictor(sd, h, rnd), defect)
    if return_at is not None:
        return preds
    return upsample(coords1 - coords0, mask_predictor(sd, h, rnd), defect)


def raft_flow_fn_ref(sd, num_flow_updates=24, dtype=torch.float64):
    """torchvision_raft's wrapper around the restatement: replicate padding to multiples of 8, [0, 1] -> [-1, 1], crop."""
    def flow_fn(src, dst):
        hh, ww = src.shape[-2:]
        ph, pw = (((hh // 8) + 1) * 8 - hh) % 8, (((ww // 8) + 1) * 8 - ww) % 8
        pad = [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2]
        a, b = (F.pad(x.to(dtype), pad, mode="replicate") * 2 - 1 for x in (src, dst))
        flow = raft_forward(sd, a, b, num_flow_updates, dtype)
        return flow[..., pad[2]:flow.shape[-2] - pad[3], pad[0]:flow.shape[-1] - pad[1]]
    return flow_fn


def make_images(n, H, W, seed=0, shift=(3.0, -2.0)):
    """Two smooth textured frames per pair in [-1, 1], the second a shifted view of the first's texture plus a little noise."""
    from dino_tracker_amd import synth
    v = synth.synth_video(2 * n, H, W, seed=seed, vx=shift[0], vy=abs(shift[1]))
    return v[0::2] * 2 - 1, v[1::2] * 2 - 1
