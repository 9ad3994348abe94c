"""CPU restatement of preprocessing/extract_trajectories.py behind its RAFT calls, in torch, in float32 or float64.

It uses the arithmetic include/dtk.h spells out for dtk_flow_*: every step is ONE ATen operation on tensors of `dtype` (so nothing
can be contracted or reordered), grid_sample(align_corners=True) written out corner by corner.  In float32 it is what the device
kernels must reproduce bit for bit; in float64 it is the yardstick for how far two fp32 evaluations may lie apart, and it can
report the smallest decision margin it met (how close any comparison or rounding came to going the other way).

`defect` plants one deviation, for the tests that show the comparison rejects it:
  "le" (<= instead of <), "round_away" (round half away from zero), "border" (border instead of zero padding in the walk and the
  masks), "no_look_behind" (a start ignores earlier trajectories), "row_order" (rows of a starting frame reversed).
"""
import torch

DEFECTS = ("le", "round_away", "border", "no_look_behind", "row_order")


class Margin:
    """the smallest distance of a decision from its boundary"""

    def __init__(self):
        self.value = float("inf")

    def see(self, dist: torch.Tensor, where: torch.Tensor = None):
        d = dist.detach().abs()
        if where is not None:
            d = d[where.expand_as(d)]
        d = d[~d.isnan()]
        if d.numel():
            self.value = min(self.value, float(d.min()))


def _src_index(x, size_m1):
    g = x * 2
    g = g / size_m1
    g = g - 1
    i = g + 1
    i = i / 2
    return i * size_m1


def _corners(img, ix, iy):
    """img [2, h, w]; ix, iy [...] source indices -> [..., 2]: the four corner terms summed from zero in the order nw, ne, sw, se"""
    h, w = img.shape[1:]
    x0, y0 = torch.floor(ix), torch.floor(iy)
    x1, y1 = x0 + 1, y0 + 1
    wx0, wx1, wy0, wy1 = x1 - ix, ix - x0, y1 - iy, iy - y0
    acc = torch.zeros(ix.shape + (2,), dtype=ix.dtype, device=ix.device)
    for xc, yc, wx, wy in ((x0, y0, wx0, wy0), (x1, y0, wx1, wy0), (x0, y1, wx0, wy1), (x1, y1, wx1, wy1)):
        ok = (xc >= 0) & (xc <= w - 1) & (yc >= 0) & (yc <= h - 1)
        xi = torch.where(ok, xc, torch.zeros_like(xc)).long()
        yi = torch.where(ok, yc, torch.zeros_like(yc)).long()
        v = img[:, yi, xi].movedim(0, -1)           # [..., 2]
        term = v * (wx * wy).unsqueeze(-1)
        acc = acc + torch.where(ok.unsqueeze(-1), term, torch.zeros_like(term))
    return acc


def bilinear(img, p, border=False):
    """img [2, h, w] sampled at the pixel coordinates p [..., 2] = (x, y); zero padding, or border padding"""
    h, w = img.shape[1:]
    ix, iy = _src_index(p[..., 0], w - 1), _src_index(p[..., 1], h - 1)
    if border:
        ix, iy = ix.clamp(0, w - 1), iy.clamp(0, h - 1)
    return _corners(img, ix, iy)


def _dist(a, b):
    d = a - b
    dx, dy = d[..., 0], d[..., 1]
    return torch.sqrt(dx * dx + dy * dy)


def _inside(p, h, w):
    return (p[..., 0] >= 0) & (p[..., 0] <= w - 1) & (p[..., 1] >= 0) & (p[..., 1] <= h - 1)


def _round(p, defect):
    if defect == "round_away":
        return torch.where(p >= 0, torch.floor(p + 0.5), torch.ceil(p - 0.5))
    return torch.round(p)


def _less(err, threshold, defect):
    return err <= threshold if defect == "le" else err < threshold


def _grid(h, w, dtype, device):
    yy, xx = torch.meshgrid(torch.arange(h, device=device), torch.arange(w, device=device), indexing="ij")
    return torch.stack((xx, yy), dim=-1).to(dtype)   # [h, w, 2]


def _mark(target, pts, defect, margin=None):
    """target [h, w] bool: set at the rounded, in-bounds positions of the non-NaN points pts [n, 2]"""
    h, w = target.shape
    pts = pts[~pts.isnan().any(-1)]
    if margin is not None:
        margin.see((pts - torch.floor(pts)) - 0.5)
    r = _round(pts, defect)
    r = r[_inside(r, h, w)].long()
    target[r[:, 1], r[:, 0]] = True


def consistency_masks(fflow, bflow, threshold, dtype=torch.float32, defect=None, margin=None):
    """get_flows_with_masks :75-93 -> [T, h, w] bool"""
    fflow, bflow = torch.as_tensor(fflow).to(dtype), torch.as_tensor(bflow).to(dtype)
    n, _, h, w = fflow.shape
    dev = fflow.device
    grid = _grid(h, w, dtype, dev)
    out = torch.zeros((n + 1, h, w), dtype=torch.bool, device=dev)
    for i in range(n):
        c1 = grid + bflow[i].permute(1, 2, 0)
        c2 = c1 + bilinear(fflow[i], c1, border=defect == "border")
        err = _dist(grid, c2)
        hit = torch.zeros((h, w), dtype=torch.bool, device=dev)
        _mark(hit, (grid + fflow[i].permute(1, 2, 0)).reshape(-1, 2), defect, margin)
        out[i + 1] = _less(err, threshold, defect) & hit
        if margin is not None:
            margin.see(err - threshold, hit)
    return out


def chain_trajectories(fflow, bflow, threshold=1.0, min_trajectory_length=2, direct_flows=None, direct_flow_threshold=None,
                       dtype=torch.float32, defect=None, margin=None, starts=None):
    """save_trajectories :195-266 -> [N, T, 2] of `dtype`, NaN where a point is not tracked.  direct_flows: s -> (forward,
    backward) [T - 1 - s, 2, h, w].  Tensors live where fflow lives.  `starts`: run only these starting frames (for timing one)."""
    assert (direct_flows is None) == (direct_flow_threshold is None)
    consistent = consistency_masks(fflow, bflow, threshold, dtype, defect, margin)
    fflow, bflow = torch.as_tensor(fflow).to(dtype), torch.as_tensor(bflow).to(dtype)
    T, h, w = fflow.shape[0] + 1, fflow.shape[2], fflow.shape[3]
    dev = fflow.device
    grid = _grid(h, w, dtype, dev)
    visited = torch.zeros((T, h, w), dtype=torch.bool, device=dev)
    border = defect == "border"
    blocks = []
    for s in (range(T - (min_trajectory_length - 1)) if starts is None else starts):
        live = ~consistent[s] | ~visited[s]
        if defect == "no_look_behind":
            live = ~consistent[s]
        traj = torch.full((h, w, T, 2), float("nan"), dtype=dtype, device=dev)
        pos = grid.clone()
        traj[:, :, s] = torch.where(live.unsqueeze(-1), pos, torch.full_like(pos, float("nan")))
        length = live.long()
        if direct_flows is not None and s < T - 1:
            dfwd, dback = (torch.as_tensor(x).to(dtype) for x in direct_flows(s))
        for k in range(T - 1 - s):
            nxt = pos + bilinear(fflow[s + k], pos, border)
            back = nxt + bilinear(bflow[s + k], nxt, border)
            err = _dist(pos, back)
            inside = _inside(nxt, h, w)
            if margin is not None:
                margin.see(err - threshold, live)
                for c, hi in ((0, w - 1), (1, h - 1)):
                    margin.see(nxt[..., c], live)
                    margin.see(nxt[..., c] - hi, live)
            step = _less(err, threshold, defect) & inside
            if direct_flows is not None:
                d = grid + dfwd[k].permute(1, 2, 0)
                d2 = d + bilinear(dback[k], d, border=True)
                derr = _dist(grid, d2)
                dmask = (_less(derr, threshold, defect) & _inside(d, h, w)).to(dtype)
                e = _dist(nxt, d) * dmask
                if margin is not None:
                    margin.see(derr - threshold, live)
                    margin.see(e - direct_flow_threshold, live & step)
                step = step & _less(e, direct_flow_threshold, defect)
            live = live & step
            pos = nxt
            traj[:, :, s + k + 1] = torch.where(live.unsqueeze(-1), pos, torch.full_like(pos, float("nan")))
            length = length + live.long()
        rows = traj.reshape(h * w, T, 2)[(length >= min_trajectory_length).reshape(-1)]
        for t in range(s, T):
            _mark(visited[t], rows[:, t], defect, margin)
        if defect == "row_order":
            rows = rows.flip(0)
        blocks.append(rows)
    return torch.cat(blocks) if blocks else torch.empty((0, T, 2), dtype=dtype, device=dev)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """the comparison the GPU tests use: same shape, same fp32 bit patterns (NaNs included)"""
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def same_pattern_within(a: torch.Tensor, b: torch.Tensor, tol: float):
    """row count and NaN pattern equal, coordinates within tol: (ok, max deviation)"""
    a, b = a.cpu().double(), b.cpu().double()
    if a.shape != b.shape or not torch.equal(a.isnan(), b.isnan()):
        return False, float("inf")
    dev = float((a - b).nan_to_num(0.0).abs().max()) if a.numel() else 0.0
    return dev <= tol, dev
