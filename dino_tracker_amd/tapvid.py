"""inference_benchmark.py's loop and eval/metrics.py's scoring without leaving the device.

  * `infer_benchmark`: the reference calls ModelInference.infer once per query START FRAME (inference_benchmark.py:36-42);
    all start frames share the refined feature volume, so here they are ONE infer() call (mixed query frames are what
    the batched pipeline handles anyway) and the result is split per frame afterwards.
  * `tapvid_metrics`: compute_tapvid_metrics_for_video (eval/metrics.py:150-223) from device tensors through
    dtk_tapvid_counts -- the five-threshold Jaccard / points-within / occlusion-accuracy numbers, no .npy round trip.
  * `badja_metrics`: compute_badja_metrics_for_video (eval/metrics.py:226-287) through dtk_badja_counts -- the segmentation-area
    threshold 0.2 sqrt(area) and the 3 px threshold, as percentages.
"""
from __future__ import annotations

from typing import Dict, Mapping, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import check, lib

THRESHOLDS = (1, 2, 4, 8, 16)


@torch.no_grad()
def infer_benchmark(model_inference, query_points: Mapping[int, Sequence], device=None,
                    batch_size=None) -> Dict[int, Tuple[torch.Tensor, torch.Tensor]]:
    """query_points {start_frame: [[x, y, start_frame], ...]} (data/tapvid.py:19-41, already at model resolution) ->
    {start_frame: (trajectories [n, T, 2], occlusions [n, T])}, the tensors inference_benchmark.py saves per frame."""
    device = device or model_inference.model.device
    frames = sorted(query_points.keys())
    parts = [torch.as_tensor(query_points[f], dtype=torch.float32, device=device).reshape(-1, 3) for f in frames]
    sizes = [p.shape[0] for p in parts]
    traj, occ = model_inference.infer(torch.cat(parts), batch_size=batch_size)
    out, pos = {}, 0
    for f, n in zip(frames, sizes):
        out[f] = (traj[pos:pos + n], occ[pos:pos + n])
        pos += n
    return out


def metrics_from_counts(counts: Sequence[int]) -> Dict[str, float]:
    """eval/metrics.py:84-146: ratios of the 18 counts, then the means over the five thresholds."""
    ev, occ_eq, vis = counts[0], counts[1], counts[2]

    def ratio(a, b):  # a video without evaluated / visible points: nan, like numpy's 0/0 in eval/metrics.py, not an exception
        return a / b if b else float("nan")

    m = {"occlusion_accuracy": ratio(occ_eq, ev)}
    fr, ja = [], []
    for i, th in enumerate(THRESHOLDS):
        correct, tp, fp = counts[3 + 3 * i], counts[4 + 3 * i], counts[5 + 3 * i]
        m[f"pts_within_{th}"] = ratio(correct, vis)
        m[f"jaccard_{th}"] = ratio(tp, vis + fp)
        fr.append(m[f"pts_within_{th}"])
        ja.append(m[f"jaccard_{th}"])
    m["average_jaccard"] = sum(ja) / len(ja)
    m["average_pts_within_thresh"] = sum(fr) / len(fr)
    return m


@torch.no_grad()
def tapvid_counts(pred_tracks: torch.Tensor, pred_occluded: torch.Tensor, gt_tracks: torch.Tensor,
                  gt_occluded: torch.Tensor, query_frames: torch.Tensor, pred_size, gt_size,
                  query_mode: str = "strided") -> torch.Tensor:
    """18 uint64 counts (dtk.h) as an int64 tensor on the device.  pred_size / gt_size = (w, h) of the rasters the two
    track sets live in; both are scaled to 256 x 256 like eval/metrics.py:204-211."""
    n, t = pred_tracks.shape[:2]
    dev = pred_tracks.device
    counts = torch.zeros(18, dtype=torch.int64, device=dev)
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731  (numpy multiplies by the float32 value)
    # locals keep the converted tensors alive until the launch is enqueued (a temporary released right after its
    # data_ptr() was taken can be handed out again by the caching allocator for the NEXT temporary)
    pt = pred_tracks.to(torch.float32).contiguous()
    po = pred_occluded.to(torch.uint8).contiguous()
    gt = gt_tracks.to(dev, torch.float32).contiguous()
    go = gt_occluded.to(dev).to(torch.uint8).contiguous()
    qf = query_frames.to(dev).to(torch.int32).contiguous()
    check(lib().dtk_tapvid_counts(ops._p(pt), ops._p(po), ops._p(gt), ops._p(go), ops._p(qf), f32(256 / pred_size[0]),
                                  f32(256 / pred_size[1]), f32(256 / gt_size[0]), f32(256 / gt_size[1]),
                                  int(query_mode == "first"), n, t, ops._p(counts), ops._stream()))
    return counts


@torch.no_grad()
def tapvid_metrics(results: Mapping[int, Tuple[torch.Tensor, torch.Tensor]], video_config: Mapping, pred_size=(854, 476),
                   query_mode: str = "strided") -> Dict[str, float]:
    """compute_tapvid_metrics_for_video (eval/metrics.py:150-223) for `results` = infer_benchmark's output and one video
    entry of the benchmark pickle ({"h", "w", "query_points", "target_points", "occluded"}, data/tapvid.py)."""
    frames = list(video_config["query_points"])
    dev = results[frames[0]][0].device
    pred = torch.cat([results[f][0][..., :2] for f in frames])
    pocc = torch.cat([results[f][1] for f in frames])
    gt = torch.cat([torch.as_tensor(video_config["target_points"][f], dtype=torch.float32) for f in frames]).to(dev)
    gocc = torch.cat([torch.as_tensor(video_config["occluded"][f].astype(bool)) for f in frames]).to(dev)
    qf = torch.cat([torch.full((len(video_config["query_points"][f]),), int(f), dtype=torch.int32) for f in frames])
    counts = tapvid_counts(pred, pocc, gt, gocc, qf, pred_size, (video_config["w"], video_config["h"]), query_mode)
    return metrics_from_counts(counts.cpu().tolist())


def metrics_from_badja_counts(counts: Sequence[int]) -> Dict[str, float]:
    """eval/metrics.py:285-287: the two means of 0 / 1 flags as percentages; nan when nothing is visible."""
    vis, seg, px3 = counts[0], counts[1], counts[2]
    return {"acc_seg": 100.0 * seg / vis if vis else float("nan"), "acc_3px": 100.0 * px3 / vis if vis else float("nan")}


@torch.no_grad()
def badja_counts(pred_tracks: torch.Tensor, gt_tracks: torch.Tensor, gt_occluded: torch.Tensor, segmentations: torch.Tensor,
                 pred_scale=(1.0, 1.0)) -> torch.Tensor:
    """3 uint64 counts (dtk.h: visible, dist < 0.2 sqrt(area[t]), dist < 3) as an int64 tensor on the device.  pred_tracks
    [N, T, 2] (taken as float32 and multiplied by float32(pred_scale) first), gt_tracks [N, T, 2] (taken as float64), gt_occluded
    [N, T] (0 = visible), segmentations [T_seg, H, W] uint8 / bool or floating (> 0 is foreground); frames 1 .. T_seg - 1 count."""
    dev = pred_tracks.device
    if pred_tracks.dim() != 3 or pred_tracks.shape[2] != 2:
        raise RuntimeError(f"dino_tracker_amd: pred_tracks must be [N, T, 2], got {tuple(pred_tracks.shape)}")
    n, t = int(pred_tracks.shape[0]), int(pred_tracks.shape[1])
    if tuple(gt_tracks.shape) != (n, t, 2) or tuple(gt_occluded.shape) != (n, t) or segmentations.dim() != 3:
        raise RuntimeError(f"dino_tracker_amd: gt_tracks {tuple(gt_tracks.shape)} / gt_occluded {tuple(gt_occluded.shape)} / "
                           f"segmentations {tuple(segmentations.shape)} do not fit pred_tracks {tuple(pred_tracks.shape)}")
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731  (numpy multiplies by the float32 value)
    # locals keep the converted tensors alive until the launches are enqueued (see tapvid_counts)
    pt = pred_tracks.to(torch.float32).contiguous()
    gt = gt_tracks.to(dev, torch.float64).contiguous()
    go = (gt_occluded.to(dev) != 0).to(torch.uint8).contiguous()
    seg = segmentations.to(dev)
    is_float = seg.is_floating_point()
    seg = (seg.to(torch.float32) if is_float else (seg > 0).to(torch.uint8) if seg.dtype != torch.uint8 else seg).contiguous()
    t_seg, h, w = (int(v) for v in seg.shape)
    areas = torch.empty(max(t_seg, 1), dtype=torch.int64, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    check(lib().dtk_badja_counts(ops._p(pt) if n else None, ops._p(gt) if n else None, ops._p(go) if n else None, ops._p(seg),
                                 int(is_float), f32(pred_scale[0]), f32(pred_scale[1]), n, t, t_seg, h, w, ops._p(areas),
                                 ops._p(counts), ops._stream()))
    return counts


@torch.no_grad()
def badja_metrics(results_or_tracks: Mapping, video_config: Mapping, pred_size=None) -> Dict[str, float]:
    """compute_badja_metrics_for_video (eval/metrics.py:226-287) for one video entry of the benchmark pickle ({"h", "w",
    "target_points", "occluded", "segmentations"}).  `results_or_tracks` is infer_benchmark's output {frame: (trajectories,
    occlusions)} or {frame: trajectories}; device tensors, or numpy arrays, which are uploaded.  Frames are concatenated over
    target_points' keys in the dict's order.  pred_size = None (predictions already in the benchmark raster) or (w, h)."""
    frames = list(video_config["target_points"])
    tracks = [results_or_tracks[f][0] if isinstance(results_or_tracks[f], (tuple, list)) else results_or_tracks[f] for f in frames]
    dev = next((x.device for x in tracks if isinstance(x, torch.Tensor)), torch.device("cuda:0"))
    pred = torch.cat([torch.as_tensor(x)[..., :2].to(dev, torch.float32) for x in tracks])
    gt = torch.cat([torch.as_tensor(np.asarray(video_config["target_points"][f], dtype=np.float64)) for f in frames])
    gocc = torch.cat([torch.as_tensor(np.asarray(video_config["occluded"][f]) != 0) for f in frames])
    seg = video_config["segmentations"]
    seg = seg if isinstance(seg, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(seg)))
    scale = (1.0, 1.0) if pred_size is None else (video_config["w"] / pred_size[0], video_config["h"] / pred_size[1])
    counts = badja_counts(pred, gt, gocc, seg, scale)
    return metrics_from_badja_counts(counts.cpu().tolist())
