"""Thin tensor-level wrappers over the C-ABI (include/dtk.h): pointer extraction, shape checks, stream hand-off.
PyTorch is used for device memory and streams only; every function here requires GPU tensors."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import Geom, TrackOpts, TrackStats, check, lib

TRACK_EXACT, TRACK_MFMA = 0, 1
TIER_AUTO, TIER_WHOLE_MAP = 0, 1


def _p(t: Optional[torch.Tensor], dtype: Optional[torch.dtype] = None):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("dino_tracker_amd: tensor is not on a GPU -- the hot path has no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError("dino_tracker_amd: tensor must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"dino_tracker_amd: expected {dtype}, got {t.dtype}")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def pack_features(chw: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[T,C,h,w] fp32 -> token-major [T,h*w,C] + per-cell norms [T,h*w]."""
    T, C, h, w = chw.shape
    thwc = torch.empty((T, h * w, C), dtype=torch.float32, device=chw.device)
    norms = torch.empty((T, h * w), dtype=torch.float32, device=chw.device)
    check(lib().dtk_pack_features(_p(chw, torch.float32), _p(thwc), _p(norms), T, C, h * w, _stream()))
    return thwc, norms


def unpack_features(thwc: torch.Tensor, h: int, w: int) -> torch.Tensor:
    T, HW, C = thwc.shape
    chw = torch.empty((T, C, h, w), dtype=torch.float32, device=thwc.device)
    check(lib().dtk_unpack_features(_p(thwc, torch.float32), _p(chw), T, C, HW, _stream()))
    return chw


def feature_norms(thwc: torch.Tensor) -> torch.Tensor:
    T, HW, C = thwc.shape
    norms = torch.empty((T, HW), dtype=torch.float32, device=thwc.device)
    check(lib().dtk_feature_norms(_p(thwc, torch.float32), _p(norms), T, C, HW, _stream()))
    return norms


def sample_points(g: Geom, feat: torch.Tensor, xy: torch.Tensor, t_idx: torch.Tensor,
                  out: Optional[torch.Tensor] = None, out_row: Optional[torch.Tensor] = None) -> torch.Tensor:
    B = xy.shape[0]
    if out is None:
        out = torch.empty((B, g.C), dtype=torch.float32, device=feat.device)
    check(lib().dtk_sample_points(g, _p(feat, torch.float32), _p(xy, torch.float32), _p(t_idx, torch.int32),
                                  _p(out_row, torch.int32), _p(out, torch.float32), B, _stream()))
    return out


def sample_grid(feat: torch.Tensor, ph: int, pw: int, pts: torch.Tensor) -> torch.Tensor:
    """utils.bilinear_interpolate_video semantics: feat token-major [T, ph*pw, C], pts [B,3] = (x, y, t) in [-1,1]."""
    T, HW, C = feat.shape
    if HW != ph * pw:
        raise RuntimeError(f"sample_grid: {HW} cells != {ph} x {pw}")
    B = pts.shape[0]
    out = torch.empty((B, C), dtype=torch.float32, device=feat.device)
    check(lib().dtk_sample_grid(_p(feat, torch.float32), T, C, ph, pw, _p(pts, torch.float32), _p(out), B, _stream()))
    return out


def normalized_conv2d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """NormalizedConv2d.forward (stride 1, padding k // 2) on the device."""
    B, Cin, H, W = x.shape
    Cout, Cin2, k, k2 = weight.shape
    if Cin2 != Cin or k != k2:
        raise RuntimeError(f"normalized_conv2d: weight {tuple(weight.shape)} does not match input {tuple(x.shape)}")
    y = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
    check(lib().dtk_normalized_conv2d(_p(x, torch.float32), _p(weight, torch.float32), _p(bias, torch.float32), _p(y), B,
                                      Cin, Cout, H, W, k, _stream()))
    return y


def corr_maps(g: Geom, feat: torch.Tensor, norms: torch.Tensor, emb: torch.Tensor, tgt: torch.Tensor,
              relu: bool = False) -> torch.Tensor:
    """Cosine maps [M, ph, pw] of emb[m] against frame tgt[m] (models/tracker.py:158-169)."""
    M = emb.shape[0]
    maps = torch.empty((M, g.ph, g.pw), dtype=torch.float32, device=feat.device)
    scratch = torch.empty(max(M, 1), dtype=torch.float32, device=feat.device)
    check(lib().dtk_corr_maps(g, _p(feat, torch.float32), _p(norms, torch.float32), _p(emb, torch.float32), None,
                              _p(tgt, torch.int32), _p(maps), _p(scratch), M, int(relu), _stream()))
    return maps


def head_prepare(sd: Dict[str, torch.Tensor], device) -> torch.Tensor:
    """TrackerHead.cnn_refiner state dict -> packed normalised parameters (dtk.h DTK_HEAD_PARAMS)."""
    w1 = sd["cnn_refiner.0.weight"].detach().to(device=device, dtype=torch.float32).contiguous()
    b1 = sd["cnn_refiner.0.bias"].detach().to(device=device, dtype=torch.float32).contiguous()
    w2 = sd["cnn_refiner.2.weight"].detach().to(device=device, dtype=torch.float32).contiguous()
    b2 = sd["cnn_refiner.2.bias"].detach().to(device=device, dtype=torch.float32).contiguous()
    if tuple(w1.shape) != (16, 1, 3, 3) or tuple(w2.shape) != (1, 16, 3, 3):
        raise RuntimeError("dino_tracker_amd: TrackerHead must be 1->16->1 with 3x3 kernels")
    head = torch.empty(305, dtype=torch.float32, device=device)
    check(lib().dtk_head_prepare(_p(w1), _p(b1), _p(w2), _p(b2), _p(head), _stream()))
    return head


def head_forward(g: Geom, head: torch.Tensor, maps: torch.Tensor, normalized: bool = True) -> torch.Tensor:
    B = maps.shape[0]
    out = torch.empty((B, 2), dtype=torch.float32, device=maps.device)
    check(lib().dtk_head_forward(g, _p(head, torch.float32), _p(maps, torch.float32), _p(out), B, int(normalized),
                                 _stream()))
    return out


def track_workspace_bytes(g: Geom, M: int, method: int, round_sources: int = 0) -> int:
    return int(lib().dtk_track_workspace_bytes(g, M, TrackOpts(method, 0, round_sources, TIER_AUTO, 0)))


def feat_f16_bytes(g: Geom) -> int:
    return int(lib().dtk_feat_f16_bytes(g))


def make_feat_f16(g: Geom, feat: torch.Tensor, norms: torch.Tensor) -> torch.Tensor:
    buf = torch.empty(feat_f16_bytes(g), dtype=torch.uint8, device=feat.device)
    check(lib().dtk_make_feat_f16(g, _p(feat, torch.float32), _p(norms, torch.float32), _p(buf), _stream()))
    return buf


def track(g: Geom, feat: torch.Tensor, norms: torch.Tensor, feat_f16: Optional[torch.Tensor], head: torch.Tensor,
          emb: torch.Tensor, src_row: Optional[torch.Tensor], tgt: torch.Tensor, out_idx: Optional[torch.Tensor],
          out_xy: torch.Tensor, M: int, workspace: torch.Tensor, dM: Optional[torch.Tensor] = None,
          normalized: bool = False, method: int = TRACK_EXACT, round_sources: int = 0, tier: int = TIER_AUTO,
          stats: Optional[TrackStats] = None) -> torch.Tensor:
    """dtk_track.  `stats` (a TrackStats) receives the tier sizes / sync count of this call."""
    opts = TrackOpts(method, int(normalized), round_sources, tier, int(emb.shape[0]) if src_row is not None else 0)
    check(lib().dtk_track(g, _p(feat, torch.float32), _p(norms, torch.float32), _p(feat_f16), _p(head, torch.float32),
                          _p(emb, torch.float32), _p(src_row, torch.int32), _p(tgt, torch.int32),
                          _p(out_idx, torch.int32), _p(out_xy, torch.float32), M, _p(dM, torch.int32), opts, stats,
                          _p(workspace), workspace.numel() * workspace.element_size(), _stream()))
    return out_xy


def argmax_cells(g: Geom, feat: torch.Tensor, norms: torch.Tensor, feat_f16: Optional[torch.Tensor], emb: torch.Tensor,
                 src_row: Optional[torch.Tensor], tgt: torch.Tensor, method: int = TRACK_MFMA,
                 workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_argmax_cells: (cell [M] int32, cosine [M] f32) of the first maximum of each source's raw cosine map."""
    M = tgt.shape[0]
    cell = torch.empty(M, dtype=torch.int32, device=feat.device)
    cos = torch.empty(M, dtype=torch.float32, device=feat.device)
    if workspace is None:
        workspace = torch.empty(track_workspace_bytes(g, M, method), dtype=torch.uint8, device=feat.device)
    check(lib().dtk_argmax_cells(g, _p(feat, torch.float32), _p(norms, torch.float32), _p(feat_f16), _p(emb, torch.float32),
                                 _p(src_row, torch.int32), _p(tgt, torch.int32), _p(cell), _p(cos), M, method,
                                 _p(workspace), workspace.numel(), _stream()))
    return cell, cos


def bb_nms(g: Geom, feat: torch.Tensor, norms: torch.Tensor, emb: torch.Tensor, src_row: Optional[torch.Tensor],
           tgt: torch.Tensor, box_size: float = 50.0, iou_thresh: float = 0.2, topk: int = 400,
           max_workspace_bytes: int = 1 << 30) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_bb_nms: (peak_affs [M, 2], r [M]) of preprocessing_dino_bb/compute_dino_bb_nms.py:12-44 for M sources."""
    M = tgt.shape[0]
    peak = torch.empty((M, 2), dtype=torch.float32, device=feat.device)
    r = torch.empty(M, dtype=torch.float32, device=feat.device)
    if M == 0:
        return peak, r
    nb = min(int(lib().dtk_bb_nms_workspace_bytes(g, M)), max_workspace_bytes)
    ws = torch.empty(nb, dtype=torch.uint8, device=feat.device)
    check(lib().dtk_bb_nms(g, _p(feat, torch.float32), _p(norms, torch.float32), _p(emb, torch.float32),
                           _p(src_row, torch.int32), _p(tgt, torch.int32), float(box_size), float(iou_thresh), int(topk),
                           _p(peak), _p(r), M, _p(ws), nb, _stream()))
    return peak, r


def _check_traj(traj: torch.Tensor) -> Tuple[int, int]:
    if traj.dim() != 3 or traj.shape[2] != 2:
        raise RuntimeError(f"dino_tracker_amd: trajectories must be [N, T, 2], got {tuple(traj.shape)}")
    if traj.shape[0] >= 2 ** 31 - 1 or traj.shape[1] == 0:
        raise RuntimeError(f"dino_tracker_amd: unsupported trajectory shape {tuple(traj.shape)}")
    return int(traj.shape[0]), int(traj.shape[1])


def traj_start_fg(traj: torch.Tensor, masks: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_traj_start_fg: (fg [N] bool, err [1] int32) -- the mask at each trajectory's first tracked point, rounded half to
    even; err counts the rows without a defined reference result (no tracked frame, start point outside the mask)."""
    N, T = _check_traj(traj)
    if masks.dim() != 3:
        raise RuntimeError(f"dino_tracker_amd: masks must be [T, H, W], got {tuple(masks.shape)}")
    Tm, H, W = masks.shape
    fg = torch.empty(N, dtype=torch.uint8, device=traj.device)
    err = torch.empty(1, dtype=torch.int32, device=traj.device)
    check(lib().dtk_traj_start_fg(_p(traj, torch.float32), N, T, _p(masks, torch.uint8), Tm, H, W, _p(fg), _p(err), _stream()))
    return fg.bool(), err


def nearest_traj(traj: torch.Tensor, gh: int, gw: int, origin: float, stride: float) -> torch.Tensor:
    """dtk_nearest_traj: idx [T, gh * gw] int32, the first trajectory at the least fp32 distance from every grid point."""
    N, T = _check_traj(traj)
    idx = torch.empty((T, gh * gw), dtype=torch.int32, device=traj.device)
    nb = int(lib().dtk_nearest_traj_workspace_bytes(N, T, gh, gw))
    ws = torch.empty(nb, dtype=torch.uint8, device=traj.device)
    check(lib().dtk_nearest_traj(_p(traj, torch.float32), N, T, gh, gw, float(origin), float(stride), _p(idx), _p(ws), nb,
                                 _stream()))
    return idx


def of_filter_keep(traj: torch.Tensor, idx: torch.Tensor, gh: int, gw: int, origin: float, stride: float, src: torch.Tensor,
                   tgt: torch.Tensor, pair_off: torch.Tensor, pair_st: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_of_filter_keep: (keep [M] bool, err [1] int32) for the best buddies of P frame pairs, concatenated (src / tgt [M, 2],
    pair_off [P + 1], pair_st [P, 2] = (source frame, target frame))."""
    N, T = _check_traj(traj)
    if N == 0:
        raise RuntimeError("dino_tracker_amd: the optical-flow filter needs at least one trajectory")
    if idx.shape != (T, gh * gw):
        raise RuntimeError(f"dino_tracker_amd: idx must be [{T}, {gh * gw}], got {tuple(idx.shape)}")
    M, P = src.shape[0], pair_st.shape[0]
    if src.shape != (M, 2) or tgt.shape != (M, 2) or pair_off.shape != (P + 1,) or pair_st.shape != (P, 2):
        raise RuntimeError("dino_tracker_amd: of_filter_keep: inconsistent src / tgt / pair_off / pair_st shapes")
    if P and not bool((pair_off[0] == 0) & (pair_off[-1] == M) & (pair_off[1:] >= pair_off[:-1]).all()):
        raise RuntimeError(f"dino_tracker_amd: of_filter_keep: pair_off must rise from 0 to {M}")
    keep = torch.empty(M, dtype=torch.uint8, device=traj.device)
    err = torch.empty(1, dtype=torch.int32, device=traj.device)
    check(lib().dtk_of_filter_keep(_p(traj, torch.float32), N, T, _p(idx, torch.int32), gh, gw, float(origin), float(stride),
                                   _p(src, torch.float32) if M else None, _p(tgt, torch.float32) if M else None,
                                   _p(pair_off, torch.int32), _p(pair_st, torch.int32), P, _p(keep), _p(err), _stream()))
    return keep.bool(), err


def flow_pack(flow: torch.Tensor) -> torch.Tensor:
    """dtk_flow_pack: planar flow fields [n, 2, h, w] -> (x, y) pairs [n, h, w, 2]."""
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise RuntimeError(f"dino_tracker_amd: flows must be [n, 2, h, w], got {tuple(flow.shape)}")
    n, _, h, w = flow.shape
    packed = torch.empty((n, h, w, 2), dtype=torch.float32, device=flow.device)
    check(lib().dtk_flow_pack(_p(flow, torch.float32) if n else None, _p(packed) if n else None, n, h, w, _stream()))
    return packed


def _check_packed(fpk: torch.Tensor, bpk: torch.Tensor) -> Tuple[int, int, int]:
    if fpk.dim() != 4 or fpk.shape[3] != 2 or bpk.shape != fpk.shape:
        raise RuntimeError(f"dino_tracker_amd: packed flows must both be [T - 1, h, w, 2], got {tuple(fpk.shape)} and "
                           f"{tuple(bpk.shape)}")
    return int(fpk.shape[0]) + 1, int(fpk.shape[1]), int(fpk.shape[2])


def flow_cycle_masks(fpk: torch.Tensor, bpk: torch.Tensor, threshold: float) -> torch.Tensor:
    """dtk_flow_cycle_masks on packed flows: consistent [T, h, w] uint8 (0 / 1)."""
    T, h, w = _check_packed(fpk, bpk)
    out = torch.empty((T, h, w), dtype=torch.uint8, device=fpk.device)
    check(lib().dtk_flow_cycle_masks(_p(fpk, torch.float32), _p(bpk, torch.float32), T, h, w, float(threshold), _p(out), _stream()))
    return out


def flow_traj_workspace(T: int, h: int, w: int, device) -> torch.Tensor:
    nb = int(lib().dtk_flow_traj_workspace_bytes(T, h, w))
    if nb == 0:
        raise RuntimeError(f"dino_tracker_amd: flow trajectories need T >= 2 and h, w >= 2, got T={T} {h}x{w}")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def flow_traj_start(fpk: torch.Tensor, bpk: torch.Tensor, consistent: torch.Tensor, visited: torch.Tensor, s: int, threshold: float,
                    min_trajectory_length: int, ws: torch.Tensor, n_rows: torch.Tensor,
                    direct: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, direct_threshold: Optional[float] = None) -> None:
    """dtk_flow_traj_start for the starting frame s; `n_rows` [1] int32 on the device receives the kept-row count.  `direct`:
    packed (forward, backward) flows s -> s + k + 1 [T - 1 - s, h, w, 2], together with `direct_threshold`."""
    T, h, w = _check_packed(fpk, bpk)
    if consistent.shape != (T, h, w) or visited.shape != (T, h, w):
        raise RuntimeError(f"dino_tracker_amd: consistent / visited must be [{T}, {h}, {w}]")
    use_direct = direct_threshold is not None
    df = db = None
    if direct is not None and T - 1 - s > 0:
        df, db = direct
        if df.shape != (T - 1 - s, h, w, 2) or db.shape != df.shape:
            raise RuntimeError(f"dino_tracker_amd: direct flows of start {s} must be [{T - 1 - s}, {h}, {w}, 2], got "
                               f"{tuple(df.shape)} and {tuple(db.shape)}")
    check(lib().dtk_flow_traj_start(_p(fpk, torch.float32), _p(bpk, torch.float32), _p(consistent, torch.uint8),
                                    _p(visited, torch.uint8), T, h, w, int(s), float(threshold), int(min_trajectory_length),
                                    _p(df, torch.float32), _p(db, torch.float32), int(use_direct),
                                    float(direct_threshold) if use_direct else 0.0, _p(n_rows, torch.int32), _p(ws),
                                    ws.numel(), _stream()))


def flow_traj_emit(T: int, h: int, w: int, s: int, min_trajectory_length: int, n_rows: int, visited: torch.Tensor,
                   ws: torch.Tensor) -> torch.Tensor:
    """dtk_flow_traj_emit: the rows [n_rows, T, 2] of the walk dtk_flow_traj_start left in `ws`; marks `visited`."""
    rows = torch.empty((n_rows, T, 2), dtype=torch.float32, device=ws.device)
    check(lib().dtk_flow_traj_emit(T, h, w, int(s), int(min_trajectory_length), int(n_rows), _p(rows) if n_rows else None,
                                   _p(visited, torch.uint8), _p(ws), ws.numel(), _stream()))
    return rows


PCA_WIDTHS, PCA_MAX_Q = (384, 768, 1024), 8


def _pca_rows(x: torch.Tensor) -> Tuple[int, int]:
    if x.dim() < 2 or x.shape[-1] not in PCA_WIDTHS or x.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: PCA input must be token-major [..., C] with C in {PCA_WIDTHS}, got {tuple(x.shape)}")
    return x.numel() // x.shape[-1], int(x.shape[-1])


def pca_moments(x: torch.Tensor, normalize: bool = True, chunk_rows: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_pca_moments: (mean [C], cov [C, C]) of the rows of a token-major fp32 volume [..., C]: cov is the centred Gram
    sum_n (x^_n - mean)(x^_n - mean)^T of the F.normalize'd rows (raw rows when not `normalize`), not divided by the row count."""
    N, C = _pca_rows(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    cov = torch.empty((C, C), dtype=torch.float32, device=x.device)
    nb = int(lib().dtk_pca_moments_workspace_bytes(N, C, int(chunk_rows)))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=x.device)
    check(lib().dtk_pca_moments(_p(x, torch.float32), N, C, int(bool(normalize)), int(chunk_rows), _p(mean), _p(cov), _p(ws), nb,
                                _stream()))
    return mean, cov


def pca_project(x: torch.Tensor, V: torch.Tensor, normalize: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_pca_project: (colors [N, q], minmax [16]) -- the (normalised, uncentred) rows of x [..., C] on the q <= 8 rows of
    V [q, C]; minmax[j] / minmax[8 + j] are the minimum / maximum of component j over all rows."""
    N, C = _pca_rows(x)
    if V.dim() != 2 or V.shape[1] != C or not 1 <= V.shape[0] <= PCA_MAX_Q:
        raise RuntimeError(f"dino_tracker_amd: V must be [q <= {PCA_MAX_Q}, {C}], got {tuple(V.shape)}")
    q = int(V.shape[0])
    colors = torch.empty((N, q), dtype=torch.float32, device=x.device)
    minmax = torch.empty(2 * PCA_MAX_Q, dtype=torch.float32, device=x.device)
    nb = int(lib().dtk_pca_project_workspace_bytes(N))
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    check(lib().dtk_pca_project(_p(x, torch.float32), N, C, int(bool(normalize)), _p(V, torch.float32), q, _p(colors), _p(minmax),
                                _p(ws), nb, _stream()))
    return colors, minmax


def fg_mask(colors: torch.Tensor, minmax: torch.Tensor, grid: Tuple[int, int, int], img_size: Tuple[int, int], threshold: float,
            comp: int = 0, flip: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_fg_mask: (mask [T, H, W], token mask [T, h, w]) uint8 0 / 255 from colors [T h w, q]: a token is foreground iff its
    min-max normalised component `comp` (one minus it when `flip`) is below `threshold`; the mask is the nearest upsampling."""
    T, h, w = (int(v) for v in grid)
    H, W = (int(v) for v in img_size)
    if colors.dim() != 2 or colors.shape[0] != T * h * w or minmax.shape != (2 * PCA_MAX_Q,):
        raise RuntimeError(f"dino_tracker_amd: fg_mask: colors {tuple(colors.shape)} / minmax {tuple(minmax.shape)} do not fit "
                           f"the grid {T}x{h}x{w}")
    mask = torch.empty((T, H, W), dtype=torch.uint8, device=colors.device)
    tok = torch.empty((T, h, w), dtype=torch.uint8, device=colors.device)
    check(lib().dtk_fg_mask(_p(colors, torch.float32), int(colors.shape[1]), int(comp), _p(minmax, torch.float32), float(threshold),
                            int(bool(flip)), T, h, w, H, W, _p(mask), _p(tok), _stream()))
    return mask, tok


def traj_cos_sims(S: torch.Tensor, tq: torch.Tensor, N: int, T: int) -> torch.Tensor:
    C = S.shape[-1]
    cs = torch.empty((N, T), dtype=torch.float32, device=S.device)
    check(lib().dtk_traj_cos_sims(_p(S, torch.float32), _p(tq, torch.int32), _p(cs), N, T, C, _stream()))
    return cs


class AnchorSources:
    """Device-side result of dtk_build_anchor_sources (worst-case sized buffers, valid prefix given by counts)."""

    def __init__(self, N: int, T: int, device):
        i32 = dict(dtype=torch.int32, device=device)
        self.N, self.T = N, T
        self.n_anchors = torch.empty(N, **i32)
        self.pair_off = torch.empty(N + 1, **i32)
        self.pair_frame = torch.empty(N * T, **i32)
        self.src_row = torch.empty(N * T * T, **i32)
        self.tgt = torch.empty(N * T * T, **i32)
        self.out_idx = torch.empty(N * T * T, **i32)
        self.counts = torch.zeros(4, **i32)
        self.scratch = torch.empty(2 * T + 2 + N, **i32)   # (the last N: dtk_build_anchor_sources_needed's per-query count)


def build_anchor_sources(cs: torch.Tensor, anchor_th: float, buf: Optional[AnchorSources] = None) -> AnchorSources:
    N, T = cs.shape
    if buf is None or buf.N != N or buf.T != T:
        buf = AnchorSources(N, T, cs.device)
    check(lib().dtk_build_anchor_sources(_p(cs, torch.float32), float(anchor_th), N, T, _p(buf.n_anchors),
                                         _p(buf.pair_off), _p(buf.pair_frame), _p(buf.src_row), _p(buf.tgt),
                                         _p(buf.out_idx), _p(buf.counts), _p(buf.scratch), _stream()))
    return buf


def build_anchor_sources_needed(cs: torch.Tensor, anchor_th: float, cos_th: float,
                                buf: Optional[AnchorSources] = None) -> AnchorSources:
    """The pairs of build_anchor_sources, but only the sources the occlusion flags depend on (include/dtk.h):
    counts = (all anchor pairs, emitted sources, queries without anchors, open queries)."""
    N, T = cs.shape
    if buf is None or buf.N != N or buf.T != T:
        buf = AnchorSources(N, T, cs.device)
    check(lib().dtk_build_anchor_sources_needed(_p(cs, torch.float32), float(anchor_th), float(cos_th), N, T,
                                                _p(buf.n_anchors), _p(buf.pair_off), _p(buf.pair_frame), _p(buf.src_row),
                                                _p(buf.tgt), _p(buf.out_idx), _p(buf.counts), _p(buf.scratch), _stream()))
    return buf


def occlusion(green: torch.Tensor, pair_off: torch.Tensor, pair_frame: torch.Tensor, traj: torch.Tensor,
              cs: torch.Tensor, anchor_th: float, cos_th: float, needed_only: bool = False) -> torch.Tensor:
    """needed_only: green holds only what build_anchor_sources_needed listed at the same thresholds (dtk_occlusion_needed)."""
    N, T = cs.shape
    occ = torch.empty((N, T), dtype=torch.uint8, device=cs.device)
    fn = lib().dtk_occlusion_needed if needed_only else lib().dtk_occlusion
    check(fn(_p(green, torch.float32), _p(pair_off, torch.int32), _p(pair_frame, torch.int32), _p(traj, torch.float32),
             _p(cs, torch.float32), float(anchor_th), float(cos_th), _p(occ), N, T, _stream()))
    return occ.bool()


def profile_enable(on: bool) -> None:
    check(lib().dtk_profile_enable(int(on)))


def profile_collect() -> Dict[str, Tuple[float, int]]:
    """{kernel name: (total ms, launches)} since profile_enable(True); synchronises."""
    n = lib().dtk_profile_collect()
    return {lib().dtk_profile_name(i).decode(): (lib().dtk_profile_ms(i), lib().dtk_profile_launches(i)) for i in range(n)}


def batchnorm_train_forward(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: Optional[torch.Tensor],
                            running_var: Optional[torch.Tensor], momentum: float, eps: float, relu: bool,
                            pre_bias: Optional[torch.Tensor] = None):
    """Train-mode BatchNorm2d (+ fused ReLU) over x [N,C,H,W]: returns (y, save_mean, save_rstd); the running statistics
    are updated in place (dtk_batchnorm_train_forward)."""
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(C, dtype=torch.float32, device=x.device)
    nb = int(lib().dtk_batchnorm_workspace_bytes(C))
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    check(lib().dtk_batchnorm_train_forward(_p(x, torch.float32), _p(gamma, torch.float32), _p(beta, torch.float32),
                                            _p(pre_bias, torch.float32), _p(running_mean, torch.float32),
                                            _p(running_var, torch.float32), float(momentum),
                                            float(eps), int(relu), _p(y), _p(mean), _p(rstd), N, C, H * W, _p(ws), nb, _stream()))
    # the kernel wrote the running statistics through raw pointers: tell torch (consumers that cache by `_version`, e.g.
    # delta_dino.weights_key -> the packed eval-mode BN constants, must see the change)
    for buf in (running_mean, running_var):
        if buf is not None:
            torch.autograd.graph.increment_version(buf)
    return y, mean, rstd


def batchnorm_train_backward(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor,
                             rstd: torch.Tensor, relu: bool, want_pre_bias: bool = False):
    """(dx, dgamma, dbeta, dpre_bias or None) of batchnorm_train_forward (dtk_batchnorm_train_backward)."""
    N, C, H, W = x.shape
    dx = torch.empty_like(x)
    dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
    dpre = torch.empty(C, dtype=torch.float32, device=x.device) if want_pre_bias else None
    nb = int(lib().dtk_batchnorm_workspace_bytes(C))
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    check(lib().dtk_batchnorm_train_backward(_p(x, torch.float32), _p(dy, torch.float32), _p(gamma, torch.float32),
                                             _p(beta, torch.float32), _p(mean, torch.float32), _p(rstd, torch.float32),
                                             int(relu), _p(dx), _p(dgamma), _p(dbeta), _p(dpre), N, C, H * W, _p(ws), nb,
                                             _stream()))
    return dx, dgamma, dbeta, dpre


def blurpool_forward(x: torch.Tensor) -> torch.Tensor:
    """BlurPool (filt 4, stride 2, reflect) of x [N,C,H,W] (dtk_blurpool_forward)."""
    N, C, H, W = x.shape
    y = torch.empty((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    check(lib().dtk_blurpool_forward(_p(x, torch.float32), _p(y), N * C, H, W, _stream()))
    return y


def blurpool_backward(dy: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Adjoint of blurpool_forward: dy [N,C,Ho,Wo] -> dx [N,C,H,W] (dtk_blurpool_backward)."""
    N, C, Ho, Wo = dy.shape
    if (Ho, Wo) != ((H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise RuntimeError(f"blurpool_backward: {Ho}x{Wo} is not the pooled size of {H}x{W}")
    dx = torch.empty((N, C, H, W), dtype=torch.float32, device=dy.device)
    check(lib().dtk_blurpool_backward(_p(dy, torch.float32), _p(dx), N * C, H, W, _stream()))
    return dx


# ---- N1: convolutions of the training step on the split-fp16 MFMA GEMM (csrc/train.hip) -----------------------------------
def gemm_nt(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, M: int, N: int, K: int, lda: int, ldb: int, ldc: int,
            batch: int = 1, stride_a: int = 0, stride_b: int = 0, stride_c: int = 0, split_k: int = 1, accumulate: int = 0,
            scale_a: Optional[torch.Tensor] = None, scale_b: Optional[torch.Tensor] = None) -> None:
    """dtk_gemm_nt_f32: C[b][m][n] (+)= sum_k A[b][m][k] B[b][n][k], fp32-grade on the fp16 matrix cores.  The tensors are
    passed as flat storage + explicit leading dimensions / batch strides (in floats); scales are 1-element device tensors."""
    check(lib().dtk_gemm_nt_f32(_p(A, torch.float32), _p(B, torch.float32), _p(C, torch.float32), M, N, K, lda, ldb, ldc, batch,
                                stride_a, stride_b, stride_c, split_k, accumulate, _p(scale_a, torch.float32),
                                _p(scale_b, torch.float32), _stream()))


def im2col(x: torch.Tensor, cols: torch.Tensor, ksize: int, pad: int, dil: int, reflect: bool, layout: int, Kp: int,
           Lp: int = 0) -> None:
    n, C, H, W = x.shape
    check(lib().dtk_im2col(_p(x, torch.float32), _p(cols, torch.float32), n, C, H, W, ksize, pad, dil, int(reflect), layout, Kp, Lp,
                           _stream()))


def col2im(dcols: torch.Tensor, dx: torch.Tensor, ksize: int, pad: int, dil: int, reflect: bool, Kp: int) -> None:
    n, C, H, W = dx.shape
    check(lib().dtk_col2im(_p(dcols, torch.float32), _p(dx, torch.float32), n, C, H, W, ksize, pad, dil, int(reflect), Kp, _stream()))


def transpose_f32(src: torch.Tensor, dst: torch.Tensor, rows: int, cols: int, batch: int = 1) -> None:
    check(lib().dtk_transpose_f32(_p(src, torch.float32), _p(dst, torch.float32), rows, cols, batch, _stream()))


def resample2d_forward(src: torch.Tensor, dst: torch.Tensor, ylo, ywhi, xlo, xwhi) -> None:
    """dtk_resample2d_forward: src [n, C, hs, ws] -> dst [n, C, hd, wd] through the per-axis two-tap tables."""
    n, c, hs, ws = src.shape
    hd, wd = dst.shape[-2:]
    check(lib().dtk_resample2d_forward(_p(src, torch.float32), _p(dst, torch.float32), n * c, hs, ws, hd, wd, _p(ylo, torch.int32),
                                       _p(ywhi, torch.float32), _p(xlo, torch.int32), _p(xwhi, torch.float32), _stream()))


def resample2d_backward(ddst: torch.Tensor, dsrc: torch.Tensor, yranges, ywhi, xranges, xwhi) -> None:
    n, c, hd, wd = ddst.shape
    hs, ws = dsrc.shape[-2:]
    check(lib().dtk_resample2d_backward(_p(ddst, torch.float32), _p(dsrc, torch.float32), n * c, hs, ws, hd, wd,
                                        _p(yranges, torch.int32), _p(ywhi, torch.float32), _p(xranges, torch.int32),
                                        _p(xwhi, torch.float32), _stream()))


def head_forward_train(g: Geom, packed_head: torch.Tensor, maps: torch.Tensor, normalized: bool = True):
    """dtk_head_forward_train: maps [B, ph*pw] (>= 0) -> (xy [B, 2], stats [B, 4])."""
    B = maps.shape[0]
    out = torch.empty((B, 2), dtype=torch.float32, device=maps.device)
    stats = torch.empty((B, 4), dtype=torch.float32, device=maps.device)
    check(lib().dtk_head_forward_train(g, _p(packed_head, torch.float32), _p(maps, torch.float32), _p(out), _p(stats), B,
                                       int(normalized), _stream()))
    return out, stats


def head_backward(g: Geom, packed_head: torch.Tensor, maps: torch.Tensor, stats: torch.Tensor, grad_out: torch.Tensor,
                  normalized: bool = True):
    """dtk_head_backward: (dmaps [B, ph*pw], dhead [305]) -- see include/dtk.h for the no-fallback condition."""
    B = maps.shape[0]
    dmaps = torch.zeros_like(maps)
    part = torch.empty((B, 305), dtype=torch.float32, device=maps.device)
    check(lib().dtk_head_backward(g, _p(packed_head, torch.float32), _p(maps, torch.float32), _p(stats, torch.float32),
                                  _p(grad_out, torch.float32), _p(dmaps), _p(part), B, int(normalized), _stream()))
    return dmaps, part.sum(dim=0)


def corr_window_backward(g: Geom, feat: torch.Tensor, norms: torch.Tensor, emb: torch.Tensor, tgt: torch.Tensor,
                         maps: torch.Tensor, dmaps: torch.Tensor, stats: torch.Tensor, dfeat: torch.Tensor) -> torch.Tensor:
    """dtk_corr_window_backward: returns demb [B, C]; accumulates into dfeat [T, ph*pw, C] (token-major)."""
    B = emb.shape[0]
    demb = torch.empty_like(emb)
    check(lib().dtk_corr_window_backward(g, _p(feat, torch.float32), _p(norms, torch.float32), _p(emb, torch.float32),
                                         _p(tgt, torch.int32), _p(maps, torch.float32), _p(dmaps, torch.float32),
                                         _p(stats, torch.float32), _p(demb), _p(dfeat, torch.float32), B, _stream()))
    return demb


def conv_split_pack(weight: torch.Tensor, flip_transpose: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_conv_split_pack: weight [Cout, Cin, 5, 5] -> (Wh, Wl) fp16 planes.  flip_transpose packs the operator of the data
    gradient (its Cin is the forward's Cout)."""
    w = weight.detach().to(torch.float32).contiguous()
    cout, cin = w.shape[:2]
    k_in, k_out = (cout, cin) if flip_transpose else (cin, cout)
    nh = int(lib().dtk_conv_split_weight_halves(k_in, k_out))
    wh = torch.empty(nh, dtype=torch.float16, device=w.device)
    wl = torch.empty(nh, dtype=torch.float16, device=w.device)
    check(lib().dtk_conv_split_pack(_p(w), k_in, k_out, int(flip_transpose), _p(wh), _p(wl), _stream()))
    return wh, wl


def conv_split_input(x: torch.Tensor, hi: torch.Tensor, lo: torch.Tensor, border: int = 0,
                     scale: Optional[torch.Tensor] = None) -> None:
    n, c, h, w = x.shape
    check(lib().dtk_conv_split_input(_p(x, torch.float32), n, c, h, w, border, _p(scale, torch.float32), _p(hi), _p(lo), _stream()))


def conv_split_run(hi: torch.Tensor, lo: torch.Tensor, wh: torch.Tensor, wl: torch.Tensor, out_nhwc: torch.Tensor, n: int, h: int,
                   w: int, cin: int, cout: int, dilation: int, zero_pad: bool, fp16_only: bool = False) -> None:
    check(lib().dtk_conv_split_run(_p(hi), _p(lo), _p(wh), _p(wl), _p(out_nhwc, torch.float32), n, h, w, cin, cout, dilation,
                                   int(zero_pad), int(fp16_only), _stream()))


def conv_split_output(y_nhwc: torch.Tensor, out: torch.Tensor, border: int = 0, reflect_fold: bool = False,
                      scale: Optional[torch.Tensor] = None) -> None:
    n, c, h, w = out.shape
    check(lib().dtk_conv_split_output(_p(y_nhwc, torch.float32), n, c, h, w, border, int(reflect_fold), _p(scale, torch.float32),
                                      _p(out, torch.float32), _stream()))


def conv_wgrad_split(x: torch.Tensor, dy: torch.Tensor, dw: torch.Tensor, dilation: int, reflect: bool,
                     scale_dy: Optional[torch.Tensor] = None, fp16_only: bool = False) -> None:
    """dtk_conv_wgrad_split: dw [Cout, Cin, 5, 5] = the weight gradient of the 5 x 5 'same' convolution (overwritten)."""
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    nb = int(lib().dtk_conv_wgrad_split_workspace_bytes(n, cin, cout, h, w, dilation))
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    check(lib().dtk_conv_wgrad_split(_p(x, torch.float32), _p(dy, torch.float32), _p(dw, torch.float32), n, cin, cout, h, w, dilation,
                                     int(reflect), _p(scale_dy, torch.float32), int(fp16_only), _p(ws), nb, _stream()))


def emb_reg_forward(x: torch.Tensor, raw: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_emb_reg_forward: x, raw [F, C, h, w] -> (out [2], per-cell sums [3, F * h * w])."""
    f, c, h, w = x.shape
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    sums = torch.empty(3, f * h * w, dtype=torch.float32, device=x.device)
    check(lib().dtk_emb_reg_forward(_p(x, torch.float32), _p(raw, torch.float32), f, c, h * w, _p(sums), _p(out), _stream()))
    return out, sums


def emb_reg_backward(x: torch.Tensor, raw: torch.Tensor, sums: torch.Tensor, gout: torch.Tensor) -> torch.Tensor:
    f, c, h, w = x.shape
    dx = torch.empty_like(x)
    check(lib().dtk_emb_reg_backward(_p(x, torch.float32), _p(raw, torch.float32), _p(sums, torch.float32), _p(gout, torch.float32),
                                     f, c, h * w, _p(dx), _stream()))
    return dx


def contrastive_forward(fe: torch.Tensor, a: torch.Tensor, fidx: torch.Tensor, temp: float):
    """dtk_contrastive_forward: fe [F, C, h, w], a [Q, B, C], fidx [Q] int32 -> (lse [Q, B], saved tensors for backward)."""
    F, C = fe.shape[:2]
    n = fe.shape[2] * fe.shape[3]
    Q, B = a.shape[:2]
    np_ = (n + 3) // 4 * 4
    dev = fe.device
    fet = torch.empty(F * n * C, dtype=torch.float32, device=dev)
    nf = torch.empty(F, n, dtype=torch.float32, device=dev)
    na = torch.empty(Q, B, dtype=torch.float32, device=dev)
    S = torch.empty(Q, B, np_, dtype=torch.float32, device=dev)
    lse = torch.empty(Q, B, dtype=torch.float32, device=dev)
    check(lib().dtk_contrastive_forward(_p(fe, torch.float32), _p(a, torch.float32), _p(fidx, torch.int32), float(temp), Q, B, C, n, F,
                                        _p(fet), _p(nf), _p(na), _p(S), _p(lse), _stream()))
    return lse, (nf, na, S)


def contrastive_backward(fe: torch.Tensor, a: torch.Tensor, fidx: torch.Tensor, temp: float, saved, lse: torch.Tensor,
                         g: torch.Tensor):
    """dtk_contrastive_backward -> (da [Q, B, C], dfe like fe)."""
    F, C = fe.shape[:2]
    n = fe.shape[2] * fe.shape[3]
    Q, B = a.shape[:2]
    nf, na, S = saved
    da = torch.empty_like(a)
    dfe = torch.empty_like(fe)
    nbytes = int(lib().dtk_contrastive_workspace_bytes(Q, B, C, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=fe.device)
    check(lib().dtk_contrastive_backward(_p(fe, torch.float32), _p(a, torch.float32), _p(fidx, torch.int32), float(temp), Q, B, C, n, F,
                                         _p(nf, torch.float32), _p(na, torch.float32), _p(S, torch.float32), _p(lse, torch.float32),
                                         _p(g, torch.float32), _p(da), _p(dfe), _p(ws), nbytes, _stream()))
    return da, dfe


# ---- track videos (csrc/render.hip, docs/RENDER.md): primitives -> tile counts -> keys -> (torch.sort) -> blend --------------------
RENDER_SEGMENT, RENDER_DISC, RENDER_DIAMOND, RENDER_RING = 0, 1, 2, 3
RENDER_DOTTED, RENDER_TAILS = 0, 1
RENDER_RECORD_WORDS, RENDER_TILE, RENDER_CHUNK = 12, 16, 256


def _render_frames(frames: torch.Tensor) -> Tuple[int, int, int]:
    if frames.dim() != 4 or frames.shape[-1] != 3 or frames.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: frames must be [F, H, W, 3] uint8, got {tuple(frames.shape)}")
    return int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])


def _render_records(records: torch.Tensor) -> int:
    if records.dim() != 2 or records.shape[1] != RENDER_RECORD_WORDS:
        raise RuntimeError(f"dino_tracker_amd: records must be [P, {RENDER_RECORD_WORDS}] float32, got {tuple(records.shape)}")
    return int(records.shape[0])


def render_prim_count(mode: int, N: int, f0: int, F: int) -> int:
    return int(lib().dtk_render_prim_count(int(mode), int(N), int(f0), int(F)))


def render_group_bytes(prims: int, keys: int, F: int, H: int, W: int) -> int:
    """dtk_render_group_bytes: device bytes of one frame group's buffers (0 for sizes the library refuses)."""
    return int(lib().dtk_render_group_bytes(int(prims), int(keys), int(F), int(H), int(W)))


def render_prims(points: torch.Tensor, occluded: torch.Tensor, colors: torch.Tensor, maps: Optional[torch.Tensor], f0: int, F: int,
                 H: int, W: int, mode: int, marker_kind: int, marker_size: float, half_width: float = 0.0,
                 trail_fade: bool = True) -> torch.Tensor:
    """dtk_render_prims: the records [P, 12] of frames f0 .. f0 + F - 1, in draw order.  points [N, T, 2] fp32, occluded [N, T]
    uint8, colors [N, 3] fp32, maps [T, T, 9] fp32 (maps[i][j] = inv(H_i) H_j) for RENDER_TAILS."""
    if points.dim() != 3 or points.shape[2] != 2 or points.shape[0] == 0:
        raise RuntimeError(f"dino_tracker_amd: points must be [N > 0, T, 2], got {tuple(points.shape)}")
    N, T = int(points.shape[0]), int(points.shape[1])
    if tuple(occluded.shape) != (N, T) or tuple(colors.shape) != (N, 3):
        raise RuntimeError(f"dino_tracker_amd: occluded {tuple(occluded.shape)} / colors {tuple(colors.shape)} do not fit "
                           f"points {tuple(points.shape)}")
    if maps is not None and tuple(maps.shape) != (T, T, 9):
        raise RuntimeError(f"dino_tracker_amd: maps must be [{T}, {T}, 9], got {tuple(maps.shape)}")
    P = render_prim_count(mode, N, f0, F)
    records = torch.empty((max(P, 0), RENDER_RECORD_WORDS), dtype=torch.float32, device=points.device)
    check(lib().dtk_render_prims(_p(points, torch.float32), _p(occluded, torch.uint8), _p(maps, torch.float32),
                                 _p(colors, torch.float32), N, T, int(f0), int(F), int(H), int(W), int(mode), int(marker_kind),
                                 float(marker_size), float(half_width), int(bool(trail_fade)), _p(records), _stream()))
    return records


def render_pred_gt_prims(pred_xy: torch.Tensor, gt_xy: torch.Tensor, pred_occluded: torch.Tensor, gt_occluded: torch.Tensor,
                         colors: torch.Tensor, f0: int, F: int, thickness: int = 4, radius: int = 8,
                         cross_size: int = 8) -> torch.Tensor:
    """dtk_render_pred_gt_prims: the records [2 N F, 12] of frames f0 .. f0 + F - 1 of a prediction-against-ground-truth video,
    two per (frame, point).  pred_xy / gt_xy [N, T, 2] int32, pred_occluded / gt_occluded [N, T] uint8, colors [N, 3] fp32."""
    if pred_xy.dim() != 3 or pred_xy.shape[2] != 2 or pred_xy.shape[0] == 0:
        raise RuntimeError(f"dino_tracker_amd: pred_xy must be [N > 0, T, 2], got {tuple(pred_xy.shape)}")
    N, T = int(pred_xy.shape[0]), int(pred_xy.shape[1])
    if (tuple(gt_xy.shape) != (N, T, 2) or tuple(pred_occluded.shape) != (N, T) or tuple(gt_occluded.shape) != (N, T)
            or tuple(colors.shape) != (N, 3)):
        raise RuntimeError(f"dino_tracker_amd: gt_xy {tuple(gt_xy.shape)} / occluded {tuple(pred_occluded.shape)}, "
                           f"{tuple(gt_occluded.shape)} / colors {tuple(colors.shape)} do not fit pred_xy {tuple(pred_xy.shape)}")
    records = torch.empty((2 * N * max(int(F), 0), RENDER_RECORD_WORDS), dtype=torch.float32, device=pred_xy.device)
    check(lib().dtk_render_pred_gt_prims(_p(pred_xy, torch.int32), _p(gt_xy, torch.int32), _p(pred_occluded, torch.uint8),
                                         _p(gt_occluded, torch.uint8), _p(colors, torch.float32), N, T, int(f0), int(F),
                                         int(thickness), int(radius), int(cross_size), _p(records), _stream()))
    return records


def render_tile_counts(records: torch.Tensor, F: int, H: int, W: int) -> torch.Tensor:
    """dtk_render_tile_counts: int32 [P], the number of 16 x 16 tiles each record's grown bounding box meets."""
    P = _render_records(records)
    counts = torch.empty(P, dtype=torch.int32, device=records.device)
    check(lib().dtk_render_tile_counts(_p(records, torch.float32), P, int(F), int(H), int(W), _p(counts), _stream()))
    return counts


def render_tile_keys(records: torch.Tensor, offsets: torch.Tensor, K: int, F: int, H: int, W: int) -> torch.Tensor:
    """dtk_render_tile_keys: int64 [K] keys (frame, tile) << 32 | record, unsorted; offsets = exclusive prefix sum of the counts."""
    P = _render_records(records)
    if tuple(offsets.shape) != (P,):
        raise RuntimeError(f"dino_tracker_amd: offsets must be [{P}], got {tuple(offsets.shape)}")
    keys = torch.empty(int(K), dtype=torch.int64, device=records.device)
    check(lib().dtk_render_tile_keys(_p(records, torch.float32), _p(offsets, torch.int64), P, int(F), int(H), int(W), int(K),
                                     _p(keys), _stream()))
    return keys


def render_tile_starts(sorted_keys: torch.Tensor, F: int, H: int, W: int) -> torch.Tensor:
    """int64 [F tiles + 1]: the first sorted key of every (frame, tile), by torch.searchsorted (plumbing)."""
    tiles = F * ((H + RENDER_TILE - 1) // RENDER_TILE) * ((W + RENDER_TILE - 1) // RENDER_TILE)
    bounds = torch.arange(tiles + 1, dtype=torch.int64, device=sorted_keys.device) << 32
    return torch.searchsorted(sorted_keys, bounds).contiguous()


def render_blend(frames: torch.Tensor, records: torch.Tensor, sorted_keys: torch.Tensor, tile_start: torch.Tensor,
                 want_float: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """dtk_render_blend: (uint8 [F, H, W, 3], fp32 [F, H, W, 3] or None)."""
    F, H, W = _render_frames(frames)
    P = _render_records(records)
    tiles = F * ((H + RENDER_TILE - 1) // RENDER_TILE) * ((W + RENDER_TILE - 1) // RENDER_TILE)
    if tuple(tile_start.shape) != (tiles + 1,):
        raise RuntimeError(f"dino_tracker_amd: tile_start must be [{tiles + 1}], got {tuple(tile_start.shape)}")
    out = torch.empty_like(frames)
    outf = torch.empty(frames.shape, dtype=torch.float32, device=frames.device) if want_float else None
    K = int(sorted_keys.numel())
    check(lib().dtk_render_blend(_p(frames, torch.uint8), _p(records, torch.float32) if P else None, P,
                                 _p(sorted_keys, torch.int64) if K else None, K, _p(tile_start, torch.int64), F, H, W, _p(out),
                                 _p(outf), _stream()))
    return out, outf


def render_records(frames: torch.Tensor, records: torch.Tensor, want_float: bool = False,
                   stats: Optional[dict] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """One frame group through bin / sort / blend.  ONE host read-back: the total key count K (the size of the key array; the
    same kind of read-back as the compacted row counts of model_inference.py).  torch.cumsum, torch.sort and torch.searchsorted
    are the plumbing between the stages."""
    F, H, W = _render_frames(frames)
    P = _render_records(records)
    _p(frames, torch.uint8)
    if P:
        counts = render_tile_counts(records, F, H, W)
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        K = int(ends[-1].item())                      # the read-back
        keys = render_tile_keys(records, (ends - counts).contiguous(), K, F, H, W)
        sorted_keys = torch.sort(keys).values if K else keys
    else:
        K, sorted_keys = 0, torch.empty(0, dtype=torch.int64, device=frames.device)
    if stats is not None:
        stats["prims"] = stats.get("prims", 0) + P
        stats["keys"] = stats.get("keys", 0) + K
        stats["groups"] = stats.get("groups", 0) + 1
    return render_blend(frames, records, sorted_keys, render_tile_starts(sorted_keys, F, H, W), want_float)


# ---- video ingest (csrc/resize.hip): Pillow's 8-bit separable resampler; the tables are video_io.lanczos_tables' ----------------
RESIZE_OUT_U8_HWC, RESIZE_OUT_F32_CHW = 0, 1
RESIZE_FORCE_GENERAL = 1
RESIZE_TILE_H, RESIZE_TILE_W = 32, 64


def resize_workspace_bytes(N: int, H: int, W: int, C: int, h: int, w: int, ksize_y: int, options: int = 0) -> int:
    """dtk_resize_workspace_bytes: bytes of the uint8 intermediate the general form needs (0: fused form, or a pass is skipped)."""
    return int(lib().dtk_resize_workspace_bytes(int(N), int(H), int(W), int(C), int(h), int(w), int(ksize_y), int(options)))


def resize_u8(frames: torch.Tensor, h: int, w: int, kx: Optional[torch.Tensor], bx: Optional[torch.Tensor],
              ky: Optional[torch.Tensor], by: Optional[torch.Tensor], u8_to_f32: Optional[torch.Tensor],
              out_form: int = RESIZE_OUT_U8_HWC, options: int = 0) -> torch.Tensor:
    """dtk_resize_u8: frames [N, H, W, C] uint8 -> uint8 [N, h, w, C] or fp32 [N, C, h, w].  k? int32 [out, ksize] weights and
    b? int32 [out, 2] bounds per axis (None for an axis whose size does not change), u8_to_f32 fp32 [256] for the fp32 form."""
    if frames.dim() != 4 or frames.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: frames must be [N, H, W, C] uint8, got {tuple(frames.shape)}")
    N, H, W, C = (int(v) for v in frames.shape)
    for k, b, n_out, axis in ((kx, bx, w, "x"), (ky, by, h, "y")):
        if k is not None and (k.dim() != 2 or k.shape[0] != n_out or b is None or tuple(b.shape) != (n_out, 2)):
            raise RuntimeError(f"dino_tracker_amd: the {axis} tables must be [{n_out}, ksize] and [{n_out}, 2], got "
                               f"{tuple(k.shape)} and {None if b is None else tuple(b.shape)}")
    if u8_to_f32 is not None and u8_to_f32.numel() != 256:
        raise RuntimeError(f"dino_tracker_amd: u8_to_f32 must hold 256 values, got {u8_to_f32.numel()}")
    ksx = int(kx.shape[1]) if kx is not None else 0
    ksy = int(ky.shape[1]) if ky is not None else 0
    if out_form == RESIZE_OUT_F32_CHW:
        out = torch.empty((N, C, int(h), int(w)), dtype=torch.float32, device=frames.device)
    else:
        out = torch.empty((N, int(h), int(w), C), dtype=torch.uint8, device=frames.device)
    nbytes = resize_workspace_bytes(N, H, W, C, h, w, ksy, options) if ky is not None else 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=frames.device) if nbytes else None
    check(lib().dtk_resize_u8(_p(frames, torch.uint8), N, H, W, C, int(h), int(w), _p(kx, torch.int32), _p(bx, torch.int32), ksx,
                              _p(ky, torch.int32), _p(by, torch.int32), ksy, _p(u8_to_f32, torch.float32), int(out_form),
                              int(options), _p(out), _p(ws), nbytes, _stream()))
    return out


# ---- video output (csrc/jpeg.hip): baseline JPEG of rendered frames; tables and header are video_out's ------------------------------
JPEG_RESTART = 16
JPEG_MCU_WORST_BYTES = 2 * 1244   # 6 blocks of at most 20 + 63 * 26 bits, every byte stuffed (docs/JPEG.md section 6)


def _jpeg_frames(frames: torch.Tensor) -> Tuple[int, int, int]:
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: frames must be [F, H, W, 3] uint8 with F, H, W >= 1, got {tuple(frames.shape)}")
    return int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])


def _jpeg_qtables(qtables: torch.Tensor):
    if tuple(qtables.shape) != (2, 64):
        raise RuntimeError(f"dino_tracker_amd: qtables must be uint8 [2, 64] (zigzag order), got {tuple(qtables.shape)}")
    return _p(qtables, torch.uint8)


def jpeg_workspace_bytes(F: int, H: int, W: int) -> int:
    """dtk_jpeg_workspace_bytes: device bytes dtk_jpeg_encode needs for F frames of H x W (0 for sizes it refuses)."""
    return int(lib().dtk_jpeg_workspace_bytes(int(F), int(H), int(W)))


def jpeg_worst_case_bytes(F: int, H: int, W: int, header_bytes: int) -> int:
    """No stream of F frames is longer: header, 2488 bytes per MCU, a marker per interval (the last one's is EOI)."""
    mcus = ((H + 15) // 16) * ((W + 15) // 16)
    return F * (header_bytes + JPEG_MCU_WORST_BYTES * mcus + 2 * ((mcus + JPEG_RESTART - 1) // JPEG_RESTART))


def jpeg_coefficients(frames: torch.Tensor, qtables: torch.Tensor) -> torch.Tensor:
    """dtk_jpeg_coefficients: frames [F, H, W, 3] uint8, qtables uint8 [2, 64] -> int16 [F, MCUs, 6, 64], zigzag order."""
    F, H, W = _jpeg_frames(frames)
    mcus = ((H + 15) // 16) * ((W + 15) // 16)
    coef = torch.empty((F, mcus, 6, 64), dtype=torch.int16, device=frames.device)
    check(lib().dtk_jpeg_coefficients(_p(frames, torch.uint8), F, H, W, _jpeg_qtables(qtables), _p(coef), _stream()))
    return coef


def jpeg_encode(frames: torch.Tensor, qtables: torch.Tensor, header: torch.Tensor,
                capacity: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_jpeg_encode: (uint8 [bytes] -- the F files one after the other --, int64 [F + 1] offsets, both on the device).
    `capacity` is the size of the first output buffer (default: the worst case); ONE host read-back, the stream's length.  When
    the stream does not fit, the call has written nothing and is repeated once with a buffer of exactly that length."""
    F, H, W = _jpeg_frames(frames)
    if header.dim() != 1 or header.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: header must be uint8 [bytes], got {tuple(header.shape)}")
    hb = int(header.numel())
    dev = frames.device
    ws = torch.empty(jpeg_workspace_bytes(F, H, W), dtype=torch.uint8, device=dev)
    offsets = torch.empty(F + 1, dtype=torch.int64, device=dev)
    needed = torch.empty(1, dtype=torch.int64, device=dev)
    cap = jpeg_worst_case_bytes(F, H, W, hb) if capacity is None else max(int(capacity), 1)
    for attempt in range(2):
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        check(lib().dtk_jpeg_encode(_p(frames, torch.uint8), F, H, W, _jpeg_qtables(qtables), _p(header, torch.uint8), hb, _p(out), cap,
                                    _p(offsets), _p(needed), _p(ws), _stream()))
        n = int(needed.item())                        # the read-back
        if n <= cap:
            return out[:n], offsets
        cap = n
    raise RuntimeError(f"dino_tracker_amd: jpeg_encode needs {n} bytes after a retry with as many")


# ---- video ingest (csrc/jpeg_decode.hip): baseline JPEG decoding; the header parser and the tables are video_in's -----------------
JPEG_SEGMENT_FIELDS = 5
JPEG_HUFF_BYTES = 272
JPEG_S_CODE, JPEG_S_INDEX, JPEG_S_OVERRUN, JPEG_S_LEFTOVER, JPEG_S_RANGE, JPEG_S_SEGMENT = 1, 2, 4, 8, 16, 32
# DTK_JPEG_*: the samplings, and per sampling (blocks per MCU, components, MCU height, MCU width)
JPEG_420, JPEG_422, JPEG_444, JPEG_GRAY = 0, 1, 2, 3
JPEG_SAMPLING_NAMES = {JPEG_420: "4:2:0", JPEG_422: "4:2:2", JPEG_444: "4:4:4", JPEG_GRAY: "grayscale"}
_JPEG_GEOMETRY = {JPEG_420: (6, 3, 16, 16), JPEG_422: (4, 3, 8, 16), JPEG_444: (3, 3, 8, 8), JPEG_GRAY: (1, 1, 8, 8)}


def jpeg_geometry(sampling: int) -> Tuple[int, int, int, int]:
    """(blocks per MCU, components, MCU height, MCU width) of a DTK_JPEG_* sampling"""
    if sampling not in _JPEG_GEOMETRY:
        raise RuntimeError(f"dino_tracker_amd: sampling must be JPEG_420, JPEG_422, JPEG_444 or JPEG_GRAY (0 .. 3), got {sampling!r}")
    return _JPEG_GEOMETRY[sampling]


def jpeg_mcus(H: int, W: int, sampling: int = JPEG_420) -> int:
    _, _, mh, mw = jpeg_geometry(sampling)
    return ((int(H) + mh - 1) // mh) * ((int(W) + mw - 1) // mw)


def jpeg_decode_workspace_bytes(F: int, H: int, W: int, sampling: int = JPEG_420) -> int:
    """dtk_jpeg_decode_workspace_bytes_sampled: device bytes dtk_jpeg_pixels_sampled needs for F frames of H x W (0 for what it
    refuses)."""
    return int(lib().dtk_jpeg_decode_workspace_bytes_sampled(int(sampling), int(F), int(H), int(W)))


def jpeg_decode_coefficients(stream: torch.Tensor, segments, huffman: torch.Tensor, H: int, W: int, sampling: int = JPEG_420
                             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_jpeg_decode_coefficients_sampled: stream uint8 [bytes] (device), segments int64 [S, 5] (a HOST array: frame, byte offset,
    byte length, first MCU, MCU count -- checked on the host, uploaded here), huffman uint8 [F, C, 2, 272] (device; C = 3
    components, 1 for JPEG_GRAY) -> (int16 [F, MCUs, B, 64] zigzag with B = 6 / 4 / 3 / 1 blocks per MCU, int32 status [F]).
    Coefficients of MCUs that no segment covers are zero."""
    import numpy as np
    B, C, _, _ = jpeg_geometry(sampling)
    seg = np.ascontiguousarray(np.asarray(segments, dtype=np.int64))
    if seg.ndim != 2 or seg.shape[1] != JPEG_SEGMENT_FIELDS or seg.shape[0] < 1:
        raise RuntimeError(f"dino_tracker_amd: segments must be int64 [S, {JPEG_SEGMENT_FIELDS}] with S >= 1, got {seg.shape}")
    if huffman.dim() != 4 or tuple(huffman.shape[1:]) != (C, 2, JPEG_HUFF_BYTES):
        raise RuntimeError(f"dino_tracker_amd: huffman must be uint8 [F, {C}, 2, {JPEG_HUFF_BYTES}], got {tuple(huffman.shape)}")
    if stream.dim() != 1 or stream.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: stream must be uint8 [bytes], got {tuple(stream.shape)}")
    F, H, W = int(huffman.shape[0]), int(H), int(W)
    mcus = jpeg_mcus(H, W, sampling)
    dev = stream.device
    coef = torch.zeros((F, mcus, B, 64), dtype=torch.int16, device=dev)
    status = torch.empty(F, dtype=torch.int32, device=dev)
    seg_dev = torch.from_numpy(seg).to(dev)
    check(lib().dtk_jpeg_decode_coefficients_sampled(int(sampling), _p(stream, torch.uint8), int(stream.numel()), _p(seg_dev),
                                                     seg.ctypes.data, int(seg.shape[0]), _p(huffman, torch.uint8), F, H, W, _p(coef),
                                                     _p(status), _stream()))
    return coef, status


def jpeg_decode_coefficients_parallel(stream: torch.Tensor, segments, huffman: torch.Tensor, H: int, W: int, sampling: int = JPEG_420,
                                      subseq_bytes: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_jpeg_decode_coefficients_parallel (csrc/jpeg_parallel.hip): jpeg_decode_coefficients with many lanes per segment -- the
    same arguments, the same coefficients and status.  subseq_bytes: the sub-stream length, 0 for the library's default, else a
    multiple of 4 in 16 .. 1024.  The segments' byte ranges must rise with the row index and not overlap."""
    import numpy as np
    B, C, _, _ = jpeg_geometry(sampling)
    seg = np.ascontiguousarray(np.asarray(segments, dtype=np.int64))
    if seg.ndim != 2 or seg.shape[1] != JPEG_SEGMENT_FIELDS or seg.shape[0] < 1:
        raise RuntimeError(f"dino_tracker_amd: segments must be int64 [S, {JPEG_SEGMENT_FIELDS}] with S >= 1, got {seg.shape}")
    if huffman.dim() != 4 or tuple(huffman.shape[1:]) != (C, 2, JPEG_HUFF_BYTES):
        raise RuntimeError(f"dino_tracker_amd: huffman must be uint8 [F, {C}, 2, {JPEG_HUFF_BYTES}], got {tuple(huffman.shape)}")
    if stream.dim() != 1 or stream.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: stream must be uint8 [bytes], got {tuple(stream.shape)}")
    F, H, W, L = int(huffman.shape[0]), int(H), int(W), int(subseq_bytes)
    need = int(lib().dtk_jpeg_decode_parallel_workspace_bytes(int(sampling), int(stream.numel()), int(seg.shape[0]), L))
    if need == 0:
        raise RuntimeError(f"dino_tracker_amd: subseq_bytes must be 0 or a multiple of 4 in 16 .. 1024, got {subseq_bytes!r}")
    mcus = jpeg_mcus(H, W, sampling)
    dev = stream.device
    coef = torch.zeros((F, mcus, B, 64), dtype=torch.int16, device=dev)
    status = torch.empty(F, dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    seg_dev = torch.from_numpy(seg).to(dev)
    check(lib().dtk_jpeg_decode_coefficients_parallel(int(sampling), _p(stream, torch.uint8), int(stream.numel()), _p(seg_dev),
                                                      seg.ctypes.data, int(seg.shape[0]), _p(huffman, torch.uint8), F, H, W, L, _p(coef),
                                                      _p(status), _p(ws), _stream()))
    return coef, status


def jpeg_pixels(coef: torch.Tensor, qtables: torch.Tensor, H: int, W: int, status: Optional[torch.Tensor] = None,
                sampling: int = JPEG_420) -> torch.Tensor:
    """dtk_jpeg_pixels_sampled: coef int16 [F, MCUs, B, 64], qtables uint8 [F, C, 64] (zigzag) -> uint8 [F, H, W, 3], for JPEG_GRAY
    uint8 [F, H, W].  `status` (int32 [F]) receives JPEG_S_RANGE for frames with |coef * Q| > 2047."""
    B, C, _, _ = jpeg_geometry(sampling)
    H, W = int(H), int(W)
    mcus = jpeg_mcus(H, W, sampling)
    if coef.dim() != 4 or tuple(coef.shape[1:]) != (mcus, B, 64) or coef.shape[0] < 1:
        raise RuntimeError(f"dino_tracker_amd: coef must be int16 [F, {mcus}, {B}, 64] for {H} x {W}, got {tuple(coef.shape)}")
    F = int(coef.shape[0])
    if tuple(qtables.shape) != (F, C, 64):
        raise RuntimeError(f"dino_tracker_amd: qtables must be uint8 [{F}, {C}, 64] (zigzag order), got {tuple(qtables.shape)}")
    if status is not None and tuple(status.shape) != (F,):
        raise RuntimeError(f"dino_tracker_amd: status must be int32 [{F}], got {tuple(status.shape)}")
    dev = coef.device
    ws = torch.empty(jpeg_decode_workspace_bytes(F, H, W, sampling), dtype=torch.uint8, device=dev)
    out = torch.empty((F, H, W) if sampling == JPEG_GRAY else (F, H, W, 3), dtype=torch.uint8, device=dev)
    check(lib().dtk_jpeg_pixels_sampled(int(sampling), _p(coef, torch.int16), _p(qtables, torch.uint8), F, H, W, _p(out),
                                        _p(status, torch.int32), _p(ws), _stream()))
    return out


JPEG_PROG_FIELDS = 14     # DTK_JPEG_PROG_FIELDS


def jpeg_decode_progressive(stream: torch.Tensor, segments, tables: torch.Tensor, frames: int, H: int, W: int,
                            sampling: int = JPEG_420) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_jpeg_decode_progressive (csrc/jpeg_progressive.hip): stream uint8 [bytes] (device), segments int64 [S, 14] (a HOST array,
    the rows dtk.h documents, ordered by level -- checked on the host, uploaded here), tables uint8 [N, 272] (device: the raw
    Huffman tables the rows name) -> (int16 [F, MCUs, B, 64] zigzag, int32 status [F]), the layout jpeg_pixels takes."""
    import numpy as np
    B, _, _, _ = jpeg_geometry(sampling)
    seg = np.ascontiguousarray(np.asarray(segments, dtype=np.int64))
    if seg.ndim != 2 or seg.shape[1] != JPEG_PROG_FIELDS or seg.shape[0] < 1:
        raise RuntimeError(f"dino_tracker_amd: segments must be int64 [S, {JPEG_PROG_FIELDS}] with S >= 1, got {seg.shape}")
    if tables.dim() != 2 or tables.shape[0] < 1 or tables.shape[1] != JPEG_HUFF_BYTES:
        raise RuntimeError(f"dino_tracker_amd: tables must be uint8 [N, {JPEG_HUFF_BYTES}] with N >= 1, got {tuple(tables.shape)}")
    if stream.dim() != 1 or stream.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: stream must be uint8 [bytes], got {tuple(stream.shape)}")
    F, H, W = int(frames), int(H), int(W)
    if F < 1:
        raise RuntimeError(f"dino_tracker_amd: frames must be positive, got {F}")
    mcus = jpeg_mcus(H, W, sampling)
    dev = stream.device
    if tables.device != dev:
        raise RuntimeError(f"dino_tracker_amd: tables are on {tables.device}, the stream on {dev}")
    coef = torch.empty((F, mcus, B, 64), dtype=torch.int16, device=dev)
    status = torch.empty(F, dtype=torch.int32, device=dev)
    seg_dev = torch.from_numpy(seg).to(dev)
    check(lib().dtk_jpeg_decode_progressive(int(sampling), _p(stream, torch.uint8), int(stream.numel()), _p(seg_dev), seg.ctypes.data,
                                            int(seg.shape[0]), _p(tables, torch.uint8), int(tables.shape[0]), F, H, W, _p(coef),
                                            _p(status), _stream()))
    return coef, status


# ---- PNG ingest (csrc/inflate.hip): zlib / DEFLATE streams, their Adler-32, the PNG row filters; the chunk parser is png_in's --------
INFLATE_STREAM_FIELDS = 4
(INFLATE_S_HEADER, INFLATE_S_BTYPE, INFLATE_S_STORED, INFLATE_S_TABLE, INFLATE_S_CODE, INFLATE_S_DISTANCE, INFLATE_S_OVERRUN,
 INFLATE_S_LENGTH, INFLATE_S_ADLER, INFLATE_S_STREAM) = (1 << k for k in range(10))
PNG_S_FILTER = 1024


def _inflate_streams(streams):
    import numpy as np
    tab = np.ascontiguousarray(np.asarray(streams, dtype=np.int64))
    if tab.ndim != 2 or tab.shape[1] != INFLATE_STREAM_FIELDS or tab.shape[0] < 1:
        raise RuntimeError(f"dino_tracker_amd: streams must be int64 [S, {INFLATE_STREAM_FIELDS}] with S >= 1, got {tab.shape}")
    return tab


def inflate(stream: torch.Tensor, streams, out_bytes: int, wrapper: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_inflate: stream uint8 [bytes] (device), streams int64 [S, 4] (a HOST array: byte offset in `stream`, byte length, byte
    offset in the output, expected output bytes -- checked on the host, uploaded here) -> (uint8 [out_bytes], int32 status [S]).
    wrapper: zlib streams (header and Adler-32 trailer; compare it with `adler32`), else raw DEFLATE."""
    tab = _inflate_streams(streams)
    if stream.dim() != 1 or stream.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: stream must be uint8 [bytes], got {tuple(stream.shape)}")
    dev = stream.device
    out = torch.empty(max(1, int(out_bytes)), dtype=torch.uint8, device=dev)
    status = torch.empty(tab.shape[0], dtype=torch.int32, device=dev)
    tab_dev = torch.from_numpy(tab).to(dev)
    check(lib().dtk_inflate(_p(stream, torch.uint8), int(stream.numel()), _p(tab_dev), tab.ctypes.data, int(tab.shape[0]),
                            1 if wrapper else 0, _p(out), int(out.numel()), _p(status), _stream()))
    return out, status


def adler32(stream: torch.Tensor, streams, out: torch.Tensor, status: torch.Tensor) -> torch.Tensor:
    """dtk_adler32: ORs INFLATE_S_ADLER into status[s] where the Adler-32 of stream s's output range differs from the big-endian value
    in the stream's last four bytes; streams whose status is already set are skipped."""
    tab = _inflate_streams(streams)
    if tuple(status.shape) != (tab.shape[0],):
        raise RuntimeError(f"dino_tracker_amd: status must be int32 [{tab.shape[0]}], got {tuple(status.shape)}")
    tab_dev = torch.from_numpy(tab).to(stream.device)
    check(lib().dtk_adler32(_p(stream, torch.uint8), int(stream.numel()), _p(tab_dev), tab.ctypes.data, int(tab.shape[0]),
                            _p(out, torch.uint8), int(out.numel()), _p(status, torch.int32), _stream()))
    return status


def png_unfilter_workspace_bytes(F: int, H: int, W: int, bpp: int) -> int:
    """dtk_png_unfilter_workspace_bytes: device bytes dtk_png_unfilter needs (0 for sizes it refuses)."""
    return int(lib().dtk_png_unfilter_workspace_bytes(int(F), int(H), int(W), int(bpp)))


def png_unfilter(raw: torch.Tensor, F: int, H: int, W: int, bpp: int, status: torch.Tensor,
                 lut: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dtk_png_unfilter: raw uint8 [F * H * (1 + W * bpp)] (filter byte + scanline per row) -> uint8 [F, H, W, bpp].  status int32
    [F] receives PNG_S_FILTER for frames with a filter byte above 4 (it is not zeroed).  lut uint8 [F, 256] (bpp = 1): the output is
    lut[f][value]."""
    F, H, W, bpp = int(F), int(H), int(W), int(bpp)
    if raw.numel() < F * H * (1 + W * bpp) or F < 1:
        raise RuntimeError(f"dino_tracker_amd: raw must hold {F} x {H} x (1 + {W} x {bpp}) bytes, got {raw.numel()}")
    if tuple(status.shape) != (F,):
        raise RuntimeError(f"dino_tracker_amd: status must be int32 [{F}], got {tuple(status.shape)}")
    if lut is not None and tuple(lut.shape) != (F, 256):
        raise RuntimeError(f"dino_tracker_amd: lut must be uint8 [{F}, 256], got {tuple(lut.shape)}")
    dev = raw.device
    ws = torch.empty(png_unfilter_workspace_bytes(F, H, W, bpp), dtype=torch.uint8, device=dev)
    out = torch.empty((F, H, W, bpp), dtype=torch.uint8, device=dev)
    check(lib().dtk_png_unfilter(_p(raw, torch.uint8), F, H, W, bpp, _p(lut, torch.uint8), _p(out), _p(status, torch.int32), _p(ws),
                                 _stream()))
    return out


# ---- PNG output (csrc/deflate.hip): the row filters, DEFLATE / zlib, the CRC-32, whole files; the IHDR is png_out's -----------------
DEFLATE_SEGMENT = 32768
DEFLATE_RANGE_FIELDS = 2
PNG_FILTER_ADAPTIVE = 5
PNG_FILE_OVERHEAD = 57          # signature + IHDR (33), the IDAT chunk's length, type and CRC (12), IEND (12)


def _png_frames(frames: torch.Tensor) -> Tuple[int, int, int, int]:
    if frames.dim() != 4 or frames.shape[3] not in (1, 3) or frames.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: frames must be [F, H, W, 1 or 3] uint8 with F, H, W >= 1, got {tuple(frames.shape)}")
    return tuple(int(v) for v in frames.shape)


def _byte_ranges(ranges):
    import numpy as np
    tab = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64))
    if tab.ndim != 2 or tab.shape[1] != DEFLATE_RANGE_FIELDS or tab.shape[0] < 1:
        raise RuntimeError(f"dino_tracker_amd: ranges must be int64 [S, {DEFLATE_RANGE_FIELDS}] with S >= 1, got {tab.shape}")
    return tab


def png_filter(frames: torch.Tensor, filter: int = PNG_FILTER_ADAPTIVE) -> torch.Tensor:
    """dtk_png_filter: frames uint8 [F, H, W, bpp] -> uint8 [F, H, 1 + W * bpp], a filter byte and the filtered scanline per row.
    filter 0 .. 4 forces one PNG filter, 5 picks per row the one with the smallest sum of |byte as int8| (ties: the lowest number)."""
    F, H, W, bpp = _png_frames(frames)
    raw = torch.empty((F, H, 1 + W * bpp), dtype=torch.uint8, device=frames.device)
    check(lib().dtk_png_filter(_p(frames, torch.uint8), F, H, W, bpp, int(filter), _p(raw), _stream()))
    return raw


def deflate_bound(n: int) -> int:
    """dtk_deflate_bound: no stream of n input bytes is longer (zlib wrapper included)"""
    return int(lib().dtk_deflate_bound(int(n)))


def deflate(data: torch.Tensor, ranges, wrapper: bool = True, capacity: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_deflate: data uint8 [bytes] (device), ranges int64 [S, 2] (a HOST array: byte offset and length of every stream's input --
    checked on the host, uploaded here) -> (uint8 [bytes] -- the S zlib or raw DEFLATE streams one after the other --, int64 [S + 1]
    offsets, both on the device).  `capacity` is the size of the first output buffer (default: the sum of the bounds, which always
    suffices); ONE host read-back, the output's length.  When the output does not fit, the call has written nothing and is repeated
    once with a buffer of exactly that length."""
    tab = _byte_ranges(ranges)
    if data.dim() != 1 or data.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: data must be uint8 [bytes], got {tuple(data.shape)}")
    S, dev = int(tab.shape[0]), data.device
    ws = torch.empty(max(1, int(lib().dtk_deflate_workspace_bytes(tab.ctypes.data, S))), dtype=torch.uint8, device=dev)
    tab_dev = torch.from_numpy(tab).to(dev)
    offsets = torch.empty(S + 1, dtype=torch.int64, device=dev)
    needed = torch.empty(1, dtype=torch.int64, device=dev)
    cap = sum(deflate_bound(max(0, int(n))) for n in tab[:, 1]) if capacity is None else max(int(capacity), 1)
    for attempt in range(2):
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        check(lib().dtk_deflate(_p(data, torch.uint8), int(data.numel()), _p(tab_dev), tab.ctypes.data, S, 1 if wrapper else 0, _p(out),
                                cap, _p(offsets), _p(needed), _p(ws), _stream()))
        n = int(needed.item())                        # the read-back
        if n <= cap:
            return out[:n], offsets
        cap = n
    raise RuntimeError(f"dino_tracker_amd: deflate needs {n} bytes after a retry with as many")


def crc32(data: torch.Tensor, ranges) -> torch.Tensor:
    """dtk_crc32: the CRC-32 (PNG / zlib) of the byte ranges int64 [S, 2] (a HOST array) of data uint8 [bytes] -> int64 [S] on the
    device, values 0 .. 2^32 - 1."""
    tab = _byte_ranges(ranges)
    if data.dim() != 1 or data.numel() == 0:
        raise RuntimeError(f"dino_tracker_amd: data must be uint8 [bytes], got {tuple(data.shape)}")
    S, dev = int(tab.shape[0]), data.device
    tab_dev = torch.from_numpy(tab).to(dev)
    out = torch.empty(S, dtype=torch.int32, device=dev)
    check(lib().dtk_crc32(_p(data, torch.uint8), int(data.numel()), _p(tab_dev), tab.ctypes.data, S, _p(out), _stream()))
    return out.to(torch.int64) & 0xFFFFFFFF


def png_encode_workspace_bytes(F: int, H: int, W: int, bpp: int) -> int:
    """dtk_png_encode_workspace_bytes: device bytes dtk_png_encode needs (0 for sizes it refuses)."""
    return int(lib().dtk_png_encode_workspace_bytes(int(F), int(H), int(W), int(bpp)))


def png_worst_case_bytes(F: int, H: int, W: int, bpp: int) -> int:
    """No F files are longer: the framing and the bound of a frame's raw scanlines."""
    return F * (PNG_FILE_OVERHEAD + deflate_bound(H * (1 + W * bpp)))


def png_encode(frames: torch.Tensor, header: torch.Tensor, filter: int = PNG_FILTER_ADAPTIVE,
               capacity: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """dtk_png_encode: frames uint8 [F, H, W, bpp], header uint8 [33] (signature + IHDR) -> (uint8 [bytes] -- the F files one after
    the other --, int64 [F + 1] offsets, both on the device).  The capacity policy is jpeg_encode's: `capacity` sizes the first output
    buffer (default: the worst case), ONE host read-back, and one retry with exactly the needed size when it was short."""
    F, H, W, bpp = _png_frames(frames)
    if tuple(header.shape) != (33,):
        raise RuntimeError(f"dino_tracker_amd: header must be uint8 [33] (signature and IHDR chunk), got {tuple(header.shape)}")
    dev = frames.device
    size = png_encode_workspace_bytes(F, H, W, bpp)
    if size == 0:
        raise RuntimeError(f"dino_tracker_amd: png_encode cannot take {F} frames of {H} x {W} x {bpp}")
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    offsets = torch.empty(F + 1, dtype=torch.int64, device=dev)
    needed = torch.empty(1, dtype=torch.int64, device=dev)
    cap = png_worst_case_bytes(F, H, W, bpp) if capacity is None else max(int(capacity), 1)
    for attempt in range(2):
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        check(lib().dtk_png_encode(_p(frames, torch.uint8), F, H, W, bpp, int(filter), _p(header, torch.uint8), _p(out), cap, _p(offsets),
                                   _p(needed), _p(ws), _stream()))
        n = int(needed.item())                        # the read-back
        if n <= cap:
            return out[:n], offsets
        cap = n
    raise RuntimeError(f"dino_tracker_amd: png_encode needs {n} bytes after a retry with as many")
