"""Track videos without matplotlib, kornia, mediapy or imageio: the reference's visualization/visualize_rainbow.py on this
implementation.

    python -m dino_tracker_amd.visualize --data-path dataset/libby --plot-trails

writes the dotted-track video (plot_tracks_v2) and, with --plot-trails, the camera-stabilised rainbow trails
(get_homographies_wrt_frame + plot_tracks_tails) into <data-path>/visualizations, the reference's file layout.

    python -m dino_tracker_amd.visualize pred-vs-gt --data-path dataset/tapvid/0 --benchmark-pickle-path davis.pkl --video-id 0

is the reference's visualization/visualize_pred_vs_gt.py without cv2: per start frame of the benchmark one video
pred_vs_gt_frame_idx_<f>_fps_<fps>.mp4 with displacement lines, discs, rings and crosses (docs/RENDER.md section 5).  The benchmark
pickle is the user's own file and is UNPICKLED: only give it files you trust.

Two halves:

* The homography estimation (get_homographies_wrt_frame and what it calls) is a float64 numpy restatement with the reference's
  signatures.  It stays on the HOST on purpose: it is T sequential frames of at most 500 eight-by-nine null-space problems whose
  decisions (RANSAC acceptance, canonical points) depend on the previous frame's result.  Every function draws from `np.random`,
  or from an `rng` argument with the same methods, the same numbers in the same order as the reference, so a seeded run
  reproduces the reference's.
* The videos are rendered on the device by csrc/render.hip (bin / sort / blend).  The picture is DEFINED in docs/RENDER.md:
  geometry, draw order and alpha rules are the reference's, the coverage model is analytic -- it is not matplotlib's Agg output
  and pixel identity with it is not claimed.  There is no CPU fallback: CPU tensors are refused; numpy arrays are uploaded.
"""
from __future__ import annotations

import argparse
import colorsys
import os
import pickle
import random
import sys
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import ops
from .utils import add_config_paths

# visualize_rainbow.py:15-23
RANSAC_INLIER_THRESHOLD = 0.07
RANSAC_TRACK_INLIER_FRAC = 0.95
NUM_REFINEMENT_PASSES = 2

FIGURE_DPI = 64                       # the reference's figure_dpi: k = 64 / 72 pixels per point (docs/RENDER.md)
PX_PER_POINT = FIGURE_DPI / 72.0
KEYS_PER_PRIM = 2                     # key-array estimate for the frame-group size: a trail segment meets 1 .. 2 tiles
DEFAULT_BUDGET = 1 << 30              # device bytes of one frame group's buffers


# ---- homographies (host, float64) -------------------------------------------------------------------------------------------------
def estimate_homography(targ_pts, src_pts, mask=None):
    """viz_utils_tapir.py:312-368: the direct linear transform; rows of masked-out points are zeroed, the solution is the right
    singular vector of the smallest singular value."""
    if mask is None:
        mask = np.ones_like(targ_pts[..., 0])
    tx, ty = targ_pts[..., 0], targ_pts[..., 1]
    sx, sy = src_pts[..., 0], src_pts[..., 1]
    one, zero = np.ones_like(tx), np.zeros_like(tx)
    rows_x = np.stack([sx, sy, one, zero, zero, zero, -tx * sx, -tx * sy, -tx], axis=-1) * mask[:, np.newaxis]
    rows_y = np.stack([zero, zero, zero, sx, sy, one, -ty * sx, -ty * sy, -ty], axis=-1) * mask[:, np.newaxis]
    a = np.concatenate([rows_x, rows_y], axis=-2)
    _, _, v = np.linalg.svd(a, full_matrices=a.shape[0] <= 8)
    return np.reshape(v[..., -1, :], (3, 3))


def compute_inliers(homog, thresh, targ_pts=None, src_pts=None, src_pts_homog=None):
    """viz_utils_tapir.py:371-386 -> (inliers, squared error, transformed points)."""
    if src_pts_homog is None:
        src_pts_homog = np.transpose(np.concatenate([src_pts, src_pts[:, 0:1] * 0 + 1], axis=-1))
    tformed = np.transpose(np.matmul(homog, src_pts_homog))
    tformed = tformed[..., :-1] / (np.maximum(1e-12, np.abs(tformed[..., -1:])) * np.sign(tformed[..., -1:]))
    err = np.sum(np.square(targ_pts - tformed), axis=-1)
    return err < thresh * thresh, err, tformed


def ransac_homography(targ_pts, src_pts, vis, thresh=4.0, targ_inlier_frac=0.5, rng=None):
    """viz_utils_tapir.py:389-441.  One rng.choice(n, 4, replace=False, p) per point, all drawn up front, as the reference."""
    rng = np.random if rng is None else rng
    n = targ_pts.shape[0]
    probs = vis / np.sum(vis)
    perm = np.array([rng.choice(n, 4, replace=False, p=probs) for _ in range(n)])
    targ_choice = np.take_along_axis(targ_pts[:, np.newaxis], perm[:, :, np.newaxis], axis=0)
    src_choice = np.take_along_axis(src_pts[:, np.newaxis], perm[:, :, np.newaxis], axis=0)
    src_homog = np.transpose(np.concatenate([src_pts, src_pts[:, 0:1] * 0 + 1], axis=-1))

    def inliers_of(h):
        return compute_inliers(h, thresh, targ_pts=targ_pts, src_pts_homog=src_homog)[0]

    it, best, homog = 0, 0, np.zeros([3, 3])
    while True:
        # the reference's stopping rule, in its float32 arithmetic: stop before the samples run out, and once the best count
        # reaches a target fraction that decays by 1 % per iteration
        threshold = np.minimum(np.array(1 - (it + 1) / src_choice.shape[0], np.float32),
                               targ_inlier_frac * (0.99 ** np.array(it, np.float32)))
        threshold = threshold * np.array(src_choice.shape[0], np.float32)
        if not np.array(best, np.float32) < threshold:
            break
        cand = estimate_homography(targ_choice[it], src_choice[it])
        count = np.sum(np.array(inliers_of(cand), np.int32))
        homog = np.where(count > best, cand, homog)
        best = np.maximum(best, count)
        it += 1
    inliers = inliers_of(homog)
    return estimate_homography(targ_pts, src_pts, np.array(inliers, np.float32)), inliers


def maybe_ransac_homography(*arg, thresh=4.0, targ_inlier_frac=0.5, rng=None):
    """viz_utils_tapir.py:444-462: RANSAC when more than four points are visible in both frames, else the identity."""
    targ_pts_all, targ_occ, src_pts_all, src_occ = arg
    vis = np.logical_and(np.logical_not(targ_occ), np.logical_not(src_occ))
    if np.sum(vis) > 4:
        final_homog, _ = ransac_homography(targ_pts_all, src_pts_all, vis, thresh, targ_inlier_frac=targ_inlier_frac, rng=rng)
    else:
        final_homog = np.eye(3)
    inliers, err, tformed = compute_inliers(final_homog, thresh, targ_pts=targ_pts_all, src_pts=src_pts_all)
    return final_homog, inliers, tformed, err


def compute_canonical_points(all_tformed, occ, err, inner_thresh, outer_thresh, required_inlier_frac, rng=None):
    """viz_utils_tapir.py:465-496.  One rng.random([n_points]) per call."""
    rng = np.random if rng is None else rng
    definite_outliers = np.logical_or(occ, err > outer_thresh)
    maybe_inliers = np.logical_and(np.logical_not(occ), err < inner_thresh)
    frac_inliers = np.sum(maybe_inliers, axis=0) / np.maximum(1.0, np.sum(np.logical_not(occ), axis=0))
    canonical_invalid = frac_inliers < required_inlier_frac
    keep = np.logical_not(definite_outliers)
    canonical_pts = np.einsum("tnc,tn->nc", all_tformed, keep) / np.maximum(1.0, np.sum(keep, axis=0)[:, np.newaxis])
    # invalid canonical points restart from a random un-occluded observation (0 when there is none)
    vis = 1 - occ
    random_choice = np.floor(rng.random([vis.shape[1]]) * np.sum(vis, axis=0))
    ids = np.cumsum(vis, axis=0) * vis - 1 * occ
    idx = ids == random_choice[np.newaxis, :]
    idx = np.sum(idx * np.arange(vis.shape[0], dtype=np.int32)[:, np.newaxis], axis=0)[np.newaxis, :, np.newaxis]
    random_pts = np.take_along_axis(all_tformed, idx, axis=0)[0]
    canonical_pts = canonical_invalid[:, np.newaxis] * random_pts + (1 - canonical_invalid[:, np.newaxis]) * canonical_pts
    return canonical_pts, canonical_invalid


def get_homographies_wrt_frame(pts, occ, image_dimensions, reference_frame=None, thresh=0.07, outlier_point_threshold=0.95,
                               targ_inlier_frac=0.7, num_refinement_passes=2, rng=None):
    """viz_utils_tapir.py:499-662 -> (homogs [T, 3, 3], err [N, T], canonical_pts [N, 2]); inv(homogs[i]) @ homogs[j] maps
    background points of frame j to frame i.  pts [N, T, 2] in pixels, occ [N, T] 0 / 1, image_dimensions [width, height]."""
    pts = np.transpose(pts, (1, 0, 2)) / np.array(image_dimensions)   # frames first, as every function above expects
    occ = np.transpose(occ)
    T = pts.shape[0]
    outer_thresh = thresh * 2.0
    if reference_frame is None:
        reference_frame = T // 2
    canonical_pts, canonical_invalid = pts[reference_frame], occ[reference_frame]
    all_tformed_pts, all_tformed_invalid, all_err = np.zeros_like(pts), np.ones_like(occ), np.zeros(occ.shape)
    all_tformed_pts[reference_frame] = canonical_pts
    all_tformed_invalid[reference_frame] = canonical_invalid
    res_homog = [None] * T
    res_homog[reference_frame] = np.eye(3)
    order = list(range(reference_frame + 1, T)) + list(range(reference_frame - 1, -1, -1))

    def canonical(err):
        return compute_canonical_points(all_tformed_pts, all_tformed_invalid, err, thresh, outer_thresh, outlier_point_threshold,
                                        rng=rng)

    for i in order:   # initial RANSAC, frame by frame away from the reference frame
        res, _, tformed, err = maybe_ransac_homography(canonical_pts, canonical_invalid, pts[i], occ[i], thresh=thresh,
                                                       targ_inlier_frac=targ_inlier_frac, rng=rng)
        all_tformed_pts[i], all_tformed_invalid[i], all_err[i], res_homog[i] = tformed, occ[i], err, res
        canonical_pts, canonical_invalid = canonical(err)
    for j in range(num_refinement_passes):
        for fr in [reference_frame] + order:
            _, err, _ = compute_inliers(res_homog[fr], thresh, canonical_pts, pts[fr])
            invalid = np.logical_or(occ[fr], np.logical_or(canonical_invalid, err > thresh * thresh))
            homog = estimate_homography(canonical_pts, pts[fr], np.array(np.logical_not(invalid), np.float32))
            if fr == reference_frame and j != num_refinement_passes - 1:
                # the reference frame's scale is pinned: its solution is applied, inverted, to every frame instead (not on the
                # last pass).  As in the reference, the transformed points land in row `fr` for every fr2 -- the last one stays.
                inv_homog = np.linalg.inv(homog)
                for fr2 in range(T):
                    res_homog[fr2] = inv_homog @ res_homog[fr2]
                    all_tformed_pts[fr] = compute_inliers(res_homog[fr2], thresh, canonical_pts, pts[fr2])[2]
                    homog = np.eye(3)
                canonical_pts, _ = canonical(all_err)
            _, err, tformed = compute_inliers(homog, thresh, canonical_pts, pts[fr])
            all_tformed_pts[fr], all_err[fr], res_homog[fr] = tformed, err, homog
            canonical_pts, canonical_invalid = canonical(err)
    scaler = np.array(list(image_dimensions) + [1])
    res_homog = res_homog @ np.diag(1.0 / scaler)
    return np.stack(res_homog, axis=0), np.transpose(all_err), canonical_pts


def filter_bg_trajectories_for_homographies(bg_trajectories, bg_trajectories_count=500, canonical_frame=None, min_len=10):
    """visualize_rainbow.py:32-54: per frame, a torch.randperm sample of the long trajectories visible there and in the canonical
    frame; the union, without duplicates."""
    N, T, _ = bg_trajectories.shape
    if canonical_frame is None:
        canonical_frame = T // 2
    valid = ~bg_trajectories.isnan().any(dim=-1)
    length = valid.sum(dim=-1)
    per_frame = bg_trajectories_count // T
    picked = []
    for t in range(T):
        both = valid[:, t] & valid[:, canonical_frame]
        idx = torch.where((length * both.float()) > min_len)[0]
        if len(idx) < per_frame:
            print(f"frame {t} and canonical frame {canonical_frame} have less than {per_frame} valid trajectories for "
                  "homography estimation.")
            idx = torch.where((length * both.float()) > 5)[0]
        picked.append(idx[torch.randperm(len(idx))[:per_frame]])
    return bg_trajectories[torch.unique(torch.stack(picked, dim=1).reshape(-1))]


def erode_mask(mask: torch.Tensor, kernel_size: int) -> torch.Tensor:
    """kornia.morphology.erosion(mask[None, None], ones(k, k)) for an ODD k: -max_pool2d(-mask, k, 1, k // 2).  The pooling's
    implicit -inf padding is kornia's geodesic border (pixels beyond the edge never lower the minimum).  An even k has an
    off-centre origin in kornia that this form does not reproduce, so it is refused.  mask [H, W] -> float [H, W]."""
    k = int(kernel_size)
    if k < 1 or k % 2 == 0:
        raise ValueError(f"erode_mask: the kernel size must be odd and positive, got {kernel_size}")
    m = mask.float()[None, None]
    return -torch.nn.functional.max_pool2d(-m, k, 1, k // 2)[0, 0]


# ---- rendering (device) -----------------------------------------------------------------------------------------------------------
def marker_size(marker: str, s: float) -> float:
    """radius of the disc 'o' / L1 radius of the diamond 'D' in pixels for matplotlib's scatter size s (points^2)."""
    if marker == "o":
        return float(np.sqrt(s) * PX_PER_POINT / 2.0)
    if marker == "D":
        return float(np.sqrt(s) * PX_PER_POINT * np.sqrt(2.0) / 2.0)
    raise NotImplementedError(f"marker {marker!r}: only 'o' and 'D' are rendered")


def rainbow_colors(N: int) -> np.ndarray:
    """colorsys.hsv_to_rgb(n / N, 1, 1): matplotlib's `hsv` map is a 256-entry table of the same ramp and differs slightly."""
    return np.array([colorsys.hsv_to_rgb(n / N, 1.0, 1.0) for n in range(N)], dtype=np.float64).reshape(N, 3)


def frame_maps(homogs) -> np.ndarray:
    """[T, T, 9] float32: inv(H_i) @ H_j formed in float64 (viz_utils_tapir.py:730), handed to the device as float32."""
    h = np.asarray(homogs.detach().cpu().numpy() if isinstance(homogs, torch.Tensor) else homogs, dtype=np.float64)
    inv = np.stack([np.linalg.inv(m) for m in h])
    return np.matmul(inv[:, None], h[None, :]).reshape(len(h), len(h), 9).astype(np.float32)


def _device_of(*xs) -> torch.device:
    for x in xs:
        if isinstance(x, torch.Tensor):
            if not x.is_cuda:
                raise RuntimeError("dino_tracker_amd: tensor is not on a GPU -- the hot path has no CPU fallback")
            return x.device
    return torch.device("cuda:0")


def _to(x, dev, dtype) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise RuntimeError("dino_tracker_amd: tensor is not on a GPU -- the hot path has no CPU fallback")
        return x.to(dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x))).to(dev).to(dtype).contiguous()


def frame_groups(mode: int, N: int, T: int, H: int, W: int, budget: int = DEFAULT_BUDGET, prim_count=None) -> list:
    """[(f0, F), ...]: consecutive frame groups whose buffers (dtk_render_group_bytes, with KEYS_PER_PRIM keys per record as the
    estimate of the key array) fit `budget` bytes; a group holds at least one frame.  `prim_count(f0, F)` replaces
    dtk_render_prim_count(mode, N, f0, F) for videos that are neither of its two modes."""
    groups, f0 = [], 0
    while f0 < T:
        F = 1
        while f0 + F < T:
            P = prim_count(f0, F + 1) if prim_count is not None else ops.render_prim_count(mode, N, f0, F + 1)
            need = ops.render_group_bytes(P, KEYS_PER_PRIM * P, F + 1, H, W)
            if need == 0 or need > budget or P >= 1 << 31:
                break
            F += 1
        groups.append((f0, F))
        f0 += F
    return groups


def _render(mode, rgb, points, occluded, maps, point_size, linewidth, marker, colors_arr, trail_fade, group_frames, budget,
            return_float, stats):
    dev = _device_of(rgb, points, occluded)
    as_numpy = not isinstance(rgb, torch.Tensor)
    if (rgb.dtype != torch.uint8) if isinstance(rgb, torch.Tensor) else (np.asarray(rgb).dtype != np.uint8):
        raise TypeError("rgb must be uint8 [T, H, W, 3]")
    frames = _to(rgb, dev, torch.uint8)
    pts = _to(points, dev, torch.float32)
    occ = _to((occluded != 0) if isinstance(occluded, torch.Tensor) else (np.asarray(occluded) != 0), dev, torch.uint8)
    T, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    N = int(pts.shape[0])
    if pts.dim() != 3 or pts.shape[1] != T or tuple(occ.shape) != (N, T):
        raise RuntimeError(f"points {tuple(pts.shape)} / occluded {tuple(occ.shape)} do not fit {T} frames")
    size = marker_size(marker, point_size)
    colors = _to(rainbow_colors(N) if colors_arr is None else colors_arr, dev, torch.float32) if N else None
    mp = _to(maps, dev, torch.float32) if maps is not None else None
    out = torch.empty_like(frames)
    outf = torch.empty(frames.shape, dtype=torch.float32, device=dev) if return_float else None
    if N == 0:
        groups = []
        out.copy_(frames)
        if outf is not None:
            outf.copy_(frames.float() / 255.0)
    elif group_frames:
        groups = [(f0, min(int(group_frames), T - f0)) for f0 in range(0, T, int(group_frames))]
    else:
        groups = frame_groups(mode, N, T, H, W, budget)
    for f0, F in groups:   # one read-back per group (ops.render_records: the key count)
        rec = ops.render_prims(pts, occ, colors, mp, f0, F, H, W, mode, ops.RENDER_DISC if marker == "o" else ops.RENDER_DIAMOND,
                               size, linewidth * PX_PER_POINT / 2.0, trail_fade)
        u8, f32 = ops.render_records(frames[f0:f0 + F], rec, return_float, stats)
        out[f0:f0 + F] = u8
        if outf is not None:
            outf[f0:f0 + F] = f32
    res = out.cpu().numpy() if as_numpy else out
    if return_float:
        return res, (outf.cpu().numpy() if as_numpy else outf)
    return res


def plot_tracks_v2(rgb, points, occluded, gt_points=None, gt_occluded=None, trackgroup=None, point_size: int = 20,
                   rainbow_colors: bool = False, marker: str = "o", colors_arr=None, show_pred_occluded=False, *,
                   group_frames: Optional[int] = None, memory_budget: int = DEFAULT_BUDGET, return_float: bool = False,
                   stats: Optional[dict] = None):
    """viz_utils_tapir.py:125-236, the form visualize_rainbow.py uses (rainbow_colors=True): one marker per point in ascending n
    at the point clamped to [0, W] x [0, H], alpha 1 - occluded.  rgb [T, H, W, 3] uint8, points [N, T, 2], occluded [N, T];
    numpy arrays or device tensors; returns [T, H, W, 3] uint8 of the kind `rgb` is."""
    if gt_points is not None or gt_occluded is not None or trackgroup is not None or show_pred_occluded or not rainbow_colors:
        raise NotImplementedError("plot_tracks_v2: gt_points / gt_occluded, trackgroup, show_pred_occluded and "
                                  "rainbow_colors=False are not rendered")
    return _render(ops.RENDER_DOTTED, rgb, points, occluded, None, point_size, 0.0, marker, colors_arr, False, group_frames,
                   memory_budget, return_float, stats)


def plot_tracks_tails(rgb, points, occluded, homogs, point_size: int = 12, linewidth: float = 1.5, marker: str = "o",
                      colors_arr=None, trail_fade: bool = True, *, group_frames: Optional[int] = None,
                      memory_budget: int = DEFAULT_BUDGET, return_float: bool = False, stats: Optional[dict] = None):
    """viz_utils_tapir.py:665-780: per frame the markers, then the trail segments of every earlier frame pair mapped into the
    frame by inv(homogs[i]) @ homogs[j], newest first, with the reference's out-of-frame rule and fade.  Frames are rendered in
    groups sized to `memory_budget` bytes (or `group_frames` frames); the result does not depend on the grouping."""
    return _render(ops.RENDER_TAILS, rgb, points, occluded, frame_maps(homogs), point_size, linewidth, marker, colors_arr,
                   trail_fade, group_frames, memory_budget, return_float, stats)


# ---- prediction against ground truth (visualization/visualize_pred_vs_gt.py) --------------------------------------------------------
def get_colors(num_colors: int, seed=0, without_red=False, rng=None) -> list:
    """viz_utils.py:7-22: one (r, g, b) of ints per point; two draws from `np.random` (or `rng`) per colour, lightness first, then
    the list is shuffled with random.seed(seed).  Reddish colours (r > 200) lose 100 of red when `without_red`."""
    rng = np.random if rng is None else rng
    colors = []
    for i in np.arange(0.0, 360.0, 360.0 / num_colors):
        hue = i / 360.0
        lightness = (50 + rng.rand() * 10) / 100.0
        saturation = (90 + rng.rand() * 10) / 100.0
        color = colorsys.hls_to_rgb(hue, lightness, saturation)
        color = (int(color[0] * 255), int(color[1] * 255), int(color[2] * 255))
        if without_red and color[0] > 200:
            color = (color[0] - 100, color[1], color[2])
        colors.append(color)
    random.seed(seed)
    random.shuffle(colors)
    return colors


COORD_LIMIT = 1 << 24   # integer coordinates beyond it are not float32 numbers; such a point is far outside any frame


def _int_points(x, dev) -> torch.Tensor:
    """tuple(point.astype(int)): truncation toward zero in the input's own dtype, as int32 on the device."""
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise RuntimeError("dino_tracker_amd: tensor is not on a GPU -- the hot path has no CPU fallback")
        t = torch.nan_to_num(x, nan=0.0) if x.is_floating_point() else x
        return t.clamp(-COORD_LIMIT, COORD_LIMIT).to(torch.int32).contiguous()
    a = np.asarray(x)
    a = np.nan_to_num(a, nan=0.0) if a.dtype.kind == "f" else a
    return torch.from_numpy(np.clip(a, -COORD_LIMIT, COORD_LIMIT).astype(int).astype(np.int32)).to(dev).contiguous()


def badja_frames(gt_trajectories) -> list:
    """visualize_pred_vs_gt.py:51: the frames where fewer than 60 % of the ground-truth points are (< 1, < 1), BADJA's mark for
    `not annotated`."""
    gt = gt_trajectories.detach().cpu().numpy() if isinstance(gt_trajectories, torch.Tensor) else np.asarray(gt_trajectories)
    return [i for i in range(gt.shape[1]) if ((gt[:, i, :] < 1).all(axis=-1)).mean() < 0.6]


def visualize_trajectories_with_gt(video, pred_trajectories, gt_trajectories, pred_occluded=None, gt_occluded=None, thickness=4,
                                   radius=8, cross_size=8, badja_vis_type=False, *, group_frames: Optional[int] = None,
                                   memory_budget: int = DEFAULT_BUDGET, return_float: bool = False,
                                   stats: Optional[dict] = None):
    """visualize_pred_vs_gt.py:40-67 on the device (docs/RENDER.md section 5).  video [T, H, W, 3] uint8, trajectories [N, T, 2],
    occlusion flags [N, T] (None: all visible); numpy arrays or device tensors.  Per frame and point, in ascending n: a red line
    prediction -> ground truth and a disc (both visible), a cross (ground truth occluded), a thin red line and a ring (prediction
    occluded), nothing (both occluded).  Colours: get_colors(N, seed=0, without_red=True) / 255, which draws from np.random as the
    reference does.  With `badja_vis_type` only the frames of badja_frames(gt) are rendered.  Returns [T', H, W, 3] uint8 of the
    kind `video` is (and the float32 picture after it with `return_float`)."""
    assert tuple(pred_trajectories.shape) == tuple(gt_trajectories.shape), \
        (f"pred and gt trajectories must be the same shape, pred.shape={tuple(pred_trajectories.shape)}, "
         f"gt.shape={tuple(gt_trajectories.shape)}")
    dev = _device_of(video, pred_trajectories, gt_trajectories, pred_occluded, gt_occluded)
    as_numpy = not isinstance(video, torch.Tensor)
    if (video.dtype != torch.uint8) if isinstance(video, torch.Tensor) else (np.asarray(video).dtype != np.uint8):
        raise TypeError("video must be uint8 [T, H, W, 3]")
    frames = _to(video, dev, torch.uint8)
    T, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    N = int(pred_trajectories.shape[0])
    if pred_trajectories.ndim != 3 or pred_trajectories.shape[2] != 2 or pred_trajectories.shape[1] < T:
        raise RuntimeError(f"trajectories {tuple(pred_trajectories.shape)} do not fit {T} frames")
    colormap = get_colors(num_colors=N, seed=0, without_red=True) if N else []
    kept = [i for i in badja_frames(gt_trajectories) if i < T] if badja_vis_type else list(range(T))

    def flags(o):
        if o is None:
            return torch.zeros((N, pred_trajectories.shape[1]), dtype=torch.uint8, device=dev)
        return _to((o != 0) if isinstance(o, torch.Tensor) else (np.asarray(o) != 0), dev, torch.uint8)

    pocc, gocc = flags(pred_occluded), flags(gt_occluded)
    if tuple(pocc.shape) != tuple(pred_trajectories.shape[:2]) or tuple(gocc.shape) != tuple(pred_trajectories.shape[:2]):
        raise RuntimeError(f"occlusion flags {tuple(pocc.shape)} / {tuple(gocc.shape)} do not fit trajectories "
                           f"{tuple(pred_trajectories.shape)}")
    idx = torch.as_tensor(kept, dtype=torch.long, device=dev)
    frames = frames.index_select(0, idx).contiguous()
    K = len(kept)
    out = frames.clone()
    outf = (frames.float() / 255.0) if return_float else None
    if N and K:
        pxy = _int_points(pred_trajectories, dev).index_select(1, idx).contiguous()
        gxy = _int_points(gt_trajectories, dev).index_select(1, idx).contiguous()
        pocc, gocc = pocc.index_select(1, idx).contiguous(), gocc.index_select(1, idx).contiguous()
        colors = _to(np.asarray(colormap, dtype=np.float64) / 255.0, dev, torch.float32)
        if group_frames:
            groups = [(f0, min(int(group_frames), K - f0)) for f0 in range(0, K, int(group_frames))]
        else:
            groups = frame_groups(-1, N, K, H, W, memory_budget, prim_count=lambda f0, F: 2 * N * F)
        for f0, F in groups:   # one read-back per group (ops.render_records: the key count)
            rec = ops.render_pred_gt_prims(pxy, gxy, pocc, gocc, colors, f0, F, thickness, radius, cross_size)
            u8, f32 = ops.render_records(frames[f0:f0 + F], rec, return_float, stats)
            out[f0:f0 + F] = u8
            if outf is not None:
                outf[f0:f0 + F] = f32
    res = out.cpu().numpy() if as_numpy else out
    if return_float:
        return res, (outf.cpu().numpy() if as_numpy else outf)
    return res


def save_video(video, path: str, fps: int = 10, container: Optional[str] = None, quality: int = 90) -> str:
    """Writes [T, H, W, 3] uint8.  container None: an mp4 through imageio when that imports; otherwise PNG frames 00000.png ... in a
    folder named like the file without its extension.  container "avi": <path without extension>.avi, a Motion-JPEG AVI, and "jpg":
    a folder of 00000.jpg ... named like the file without its extension -- both through the device JPEG encoder (video_out.py) at
    `quality`.  container "png": a folder of 00000.png ... through the device PNG encoder (png_out.py), lossless.  A device tensor
    is encoded where it is, without a trip to the host.  Returns what it wrote and says so."""
    if container is not None:
        from . import video_out
        if container not in ("avi", "jpg", "png"):
            raise ValueError(f"save_video: container must be None, 'avi', 'jpg' or 'png', got {container!r}")
        stem, frames = os.path.splitext(path)[0], len(video)
        if container == "png":
            from . import png_out
            written = png_out.write_png_frames(video, stem)
            print(f"save_video: wrote {frames} PNG frames (device encoder, lossless) to {written}/")
        elif container == "avi":
            written = video_out.write_mjpeg_avi(video, stem + ".avi", fps=fps, quality=quality)
            print(f"save_video: wrote {written} (Motion-JPEG avi, {frames} frames, {fps} fps, quality {quality}, "
                  f"{os.path.getsize(written)} bytes)")
        else:
            written = video_out.write_jpeg_frames(video, stem, quality=quality)
            print(f"save_video: wrote {frames} JPEG frames (quality {quality}) to {written}/")
        return written
    video = video.cpu().numpy() if isinstance(video, torch.Tensor) else np.asarray(video)
    try:
        import imageio
    except ImportError:
        imageio = None
    if imageio is not None:
        writer = imageio.get_writer(path, fps=fps)
        for frame in video:
            writer.append_data(frame)
        writer.close()
        print(f"save_video: wrote {path} (mp4, {len(video)} frames, {fps} fps)")
        return path
    from PIL import Image
    folder = os.path.splitext(path)[0]
    os.makedirs(folder, exist_ok=True)
    for i, frame in enumerate(video):
        Image.fromarray(frame).save(os.path.join(folder, f"{i:05d}.png"))
    print(f"save_video: imageio is not installed -- wrote {len(video)} PNG frames to {folder}/ instead of {path}")
    return folder


def _load_video_u8(video_folder: str, num_frames: Optional[int] = 300) -> np.ndarray:
    from PIL import Image
    files = sorted(list(Path(video_folder).glob("*.jpg")) + list(Path(video_folder).glob("*.png")))[:num_frames]
    return np.stack([np.asarray(Image.open(str(f)).convert("RGB")) for f in files])


def _container_args(args) -> dict:
    """--container / --quality as save_video's keywords; `auto` (and an args object without the flags) is save_video's default"""
    container = getattr(args, "container", "auto")
    return {"container": None if container == "auto" else container, "quality": getattr(args, "quality", 90)}


def _add_container_flags(p: argparse.ArgumentParser) -> None:
    p.add_argument("--container", choices=("auto", "avi", "jpg", "png"), default="auto",
                   help="auto: mp4 through imageio, PNG frames without it; avi: Motion-JPEG AVI, jpg: a folder of JPEG frames and "
                        "png: a folder of PNG frames (lossless), all three encoded on the device")
    p.add_argument("--quality", type=int, default=90, help="JPEG quality 1 .. 100 of --container avi / jpg")


@torch.no_grad()
def run(args, device: str = "cuda:0"):
    """visualize_rainbow.py:57-142 on the layout of utils.add_config_paths."""
    from PIL import Image
    paths = add_config_paths(args.data_path, {})
    masks_path = Path(paths["masks_path"])
    mask_file = sorted(list(masks_path.glob("*.jpg")) + list(masks_path.glob("*.png")))[args.vis_start_frame]
    out_dir = paths["model_vis_dir"]
    video = _load_video_u8(paths["video_folder"])
    H, W = video.shape[1], video.shape[2]
    tracks = np.load(os.path.join(paths["grid_trajectories_dir"], "grid_trajectories.npy"))
    if args.infer_res_size is not None:
        ph, pw = args.infer_res_size
        tracks = tracks * np.array([W / pw, H / ph], dtype=np.float32)
    occ_path = os.path.join(paths["grid_occlusions_dir"], "grid_occlusions.npy")
    if os.path.isfile(occ_path):
        occluded = np.load(occ_path).astype(np.int32)
    else:
        print(f"{occ_path} does not exist, marking all points as visible ---")
        occluded = np.zeros(tracks.shape[:-1], dtype=np.int32)
    mask = torch.from_numpy(np.array(Image.open(mask_file).convert("L"))).bool().float()
    if tuple(mask.shape) != (H, W):
        mask = torch.nn.functional.interpolate(mask[None, None], size=(H, W), mode="nearest")[0, 0]
    if args.erosion_kernel_size is not None:
        mask = erode_mask(mask, args.erosion_kernel_size).bool()
    mask = mask.numpy()
    coords = tracks[:, 0].round().astype(np.int32)
    is_fg = mask[coords[:, 1], coords[:, 0]] > 0
    start = args.vis_start_frame
    end = args.vis_end_frame if args.vis_end_frame is not None else video.shape[0]
    video, tracks, occluded = video[start:end], tracks[:, start:end], occluded[:, start:end]
    os.makedirs(out_dir, exist_ok=True)
    ero = args.erosion_kernel_size
    name = f"dotted_tracks_fps_{args.fps}.mp4" if ero is None else f"dotted_tracks_erosion_kernel_{ero}_fps_{args.fps}.mp4"
    frames = torch.from_numpy(video).to(device)
    dotted = plot_tracks_v2(frames, tracks[is_fg], occluded[is_fg], rainbow_colors=True, point_size=args.point_size)
    how = _container_args(args)
    written = [save_video(dotted, os.path.join(out_dir, name), fps=args.fps, **how)]
    if args.plot_trails:
        bg = torch.load(paths["bg_trajectories_file"], map_location="cpu")[:, start:end]
        bg = filter_bg_trajectories_for_homographies(bg, canonical_frame=args.canonical_frame)
        bg_occ = bg.isnan().any(dim=-1).int().numpy()
        oh, ow = args.of_res_size
        bg = np.nan_to_num(bg.numpy(), nan=0) * np.array([W / ow, H / oh], dtype=np.float32)
        homogs, _, _ = get_homographies_wrt_frame(bg, bg_occ, [W, H], thresh=RANSAC_INLIER_THRESHOLD,
                                                  outlier_point_threshold=RANSAC_TRACK_INLIER_FRAC,
                                                  num_refinement_passes=NUM_REFINEMENT_PASSES, reference_frame=args.canonical_frame)
        rainbow = plot_tracks_tails(frames, tracks[is_fg], occluded[is_fg], homogs, point_size=args.point_size,
                                    linewidth=args.linewidth, marker="D")
        name = f"rainbow_fps_{args.fps}.mp4" if ero is None else f"rainbow_erosion_kernel_{ero}_fps_{args.fps}.mp4"
        written.append(save_video(rainbow, os.path.join(out_dir, name), fps=args.fps, **how))
    print("Saved to", out_dir)
    return written


@torch.no_grad()
def save_prediction_vs_gt(args, device: str = "cuda:0"):
    """visualize_pred_vs_gt.py:70-106 on the layout of utils.add_config_paths: per start frame of the benchmark video one
    pred_vs_gt_frame_idx_<f>_fps_<fps>.mp4 (or PNG folder, .avi or JPEG folder, see save_video) in <data-path>/visualizations."""
    paths = add_config_paths(args.data_path, {})
    with open(args.benchmark_pickle_path, "rb") as fh:
        benchmark_data = pickle.load(fh)
    config = next((v for v in benchmark_data["videos"] if v["video_idx"] == args.video_id), None)
    orig_h, orig_w = config["h"], config["w"]
    frames = torch.from_numpy(_load_video_u8(paths["video_folder"], None)).to(device)
    pred_h, pred_w = args.infer_res_size
    out_dir = paths["model_vis_dir"]
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for idx, frame_idx in enumerate(sorted(config["target_points"].keys())):
        if idx > 0 and args.only_first_frame:
            break
        gt = np.array(config["target_points"][frame_idx])
        gt_occ = np.array(config["occluded"][frame_idx])
        pred = np.load(os.path.join(paths["trajectories_dir"], f"trajectories_{frame_idx}.npy"))
        pred = pred * np.array([orig_w / pred_w, orig_h / pred_h], dtype=np.float32)   # to the video's resolution
        if args.use_gt_occ:
            pred_occ = gt_occ
        else:
            occ_file = os.path.join(paths["occlusions_dir"], f"occlusion_preds_{frame_idx}.npy")
            assert os.path.exists(occ_file), f"occlusion_preds_{frame_idx}.npy does not exist"
            pred_occ = np.load(occ_file)
        video = visualize_trajectories_with_gt(frames, pred, gt, pred_occ, gt_occ, badja_vis_type=args.badja_vis_type)
        written.append(save_video(video, os.path.join(out_dir, f"pred_vs_gt_frame_idx_{frame_idx}_fps_{args.fps}.mp4"), fps=args.fps,
                                  **_container_args(args)))
    print("Saved to", out_dir)
    return written


def make_pred_vs_gt_parser() -> argparse.ArgumentParser:
    """visualize_pred_vs_gt.py:109-118, argument for argument."""
    p = argparse.ArgumentParser(prog="python -m dino_tracker_amd.visualize pred-vs-gt",
                                description="prediction-against-ground-truth videos of a benchmark video")
    p.add_argument("--data-path", default="./dataset/libby", type=str, required=True)
    p.add_argument("--benchmark-pickle-path", type=str, required=True, help="the benchmark file; it is unpickled")
    p.add_argument("--video-id", type=int, required=True)
    p.add_argument("--infer-res-size", type=int, nargs=2, default=(476, 854), help="inference resolution (h, w), as in train.yaml")
    p.add_argument("--badja-vis-type", action="store_true", help="render only the frames with ground-truth annotations (BADJA)")
    p.add_argument("--only-first-frame", action="store_true", help="only the query points of the first start frame")
    p.add_argument("--use-gt-occ", action="store_true", help="use the ground-truth occlusion for the predictions too")
    p.add_argument("--fps", type=int, default=10, help="fps=10 for TAP-Vid, fps=2 for BADJA")
    _add_container_flags(p)
    return p


def make_parser() -> argparse.ArgumentParser:
    """visualize_rainbow.py:145-158, argument for argument."""
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--data-path", default="./dataset/libby", type=str)
    p.add_argument("--infer-res-size", type=int, nargs=2, default=(476, 854), help="inference resolution (h, w), as in train.yaml")
    p.add_argument("--of-res-size", type=int, nargs=2, default=(476, 854), help="optical-flow resolution (h, w), as in preprocess.yaml")
    p.add_argument("--erosion-kernel-size", type=int, default=None, help="odd size of the mask erosion kernel; none when omitted")
    p.add_argument("--vis-start-frame", type=int, default=0, help="same as start_frame of inference_grid.py")
    p.add_argument("--vis-end-frame", type=int, default=None)
    p.add_argument("--canonical-frame", type=int, default=None)
    p.add_argument("--fps", type=int, default=10)
    p.add_argument("--point-size", type=int, default=40)
    p.add_argument("--linewidth", type=float, default=1.5)
    p.add_argument("--plot-trails", action="store_true", default=False, help="also render the rainbow trails (needs homographies)")
    _add_container_flags(p)
    return p


def main(argv=None):
    """`pred-vs-gt` as the first argument selects save_prediction_vs_gt; everything else is the track-video command line."""
    argv = sys.argv[1:] if argv is None else list(argv)
    if argv[:1] == ["pred-vs-gt"]:
        return save_prediction_vs_gt(make_pred_vs_gt_parser().parse_args(argv[1:]))
    return run(make_parser().parse_args(argv))


if __name__ == "__main__":
    main()
