"""Dataset evaluation without pandas: the reference's eval/eval_benchmark.py on this implementation.

    python -m dino_tracker_amd.evaluate --dataset-root-dir dataset/davis_256 --benchmark-pickle-path dataset/davis.pkl \\
        --out-file tapvid/comp_metrics.csv --dataset-type tapvid
    python -m dino_tracker_amd.evaluate --dataset-root-dir dataset/badja --benchmark-pickle-path dataset/badja.pkl \\
        --out-file badja/comp_metrics.csv --dataset-type BADJA

For every sub-folder <video_idx> of the dataset root that does not start with a dot it loads what inference_benchmark.py saved
(trajectories/trajectories_<f>.npy and, for tapvid, occlusions/occlusion_preds_<f>.npy), uploads the arrays and scores them on the
device through dtk_tapvid_counts or dtk_badja_counts (dino_tracker_amd/tapvid.py).  The CSV has the reference's layout: the header
`video_idx` + the metric names in the order of the reference's dict, one row per video, and a last row `average` with the column
means, NaNs skipped (DataFrame.mean's rule; an empty field stands for NaN, as in DataFrame.to_csv).

--benchmark-pickle-path is the user's own benchmark file and is UNPICKLED (pickle.load): only give it files you trust.
"""
from __future__ import annotations

import argparse
import csv
import math
import os
import pickle
from typing import Callable, Dict, List, Mapping, Optional

import numpy as np
import torch

from . import tapvid


def get_video_config_by_video_id(benchmark_config: Mapping, video_id: int):
    """data/tapvid.py:5-16."""
    for video_config in benchmark_config["videos"]:
        if video_config["video_idx"] == video_id:
            return video_config
    return None


def _load(path: str, device) -> torch.Tensor:
    assert os.path.exists(path), f"failed to load {path}"
    return torch.from_numpy(np.load(path)).to(device)


def tapvid_video_metrics(trajectories_dir: str, occlusions_dir: str, video_config: Mapping, pred_video_sizes,
                         device="cuda:0") -> Dict[str, float]:
    """compute_tapvid_metrics_for_video (eval/metrics.py:150-223) from the .npy files of one video."""
    results = {}
    for f in video_config["query_points"]:
        traj = _load(os.path.join(trajectories_dir, f"trajectories_{f}.npy"), device)
        occ = _load(os.path.join(occlusions_dir, f"occlusion_preds_{f}.npy"), device)
        results[f] = (traj, occ)
    size = (video_config["w"], video_config["h"]) if pred_video_sizes is None else tuple(pred_video_sizes)
    return tapvid.tapvid_metrics(results, video_config, pred_size=size)


def badja_video_metrics(trajectories_dir: str, video_config: Mapping, pred_video_sizes, device="cuda:0") -> Dict[str, float]:
    """compute_badja_metrics_for_video (eval/metrics.py:226-287) from the .npy files of one video."""
    results = {f: _load(os.path.join(trajectories_dir, f"trajectories_{f}.npy"), device) for f in video_config["target_points"]}
    return tapvid.badja_metrics(results, video_config, None if pred_video_sizes is None else tuple(pred_video_sizes))


def column_means(rows: List[Mapping[str, float]], names: List[str]) -> Dict[str, float]:
    """DataFrame.mean: per column, the mean of the values that are not NaN; NaN when there is none."""
    out = {}
    for name in names:
        vals = [float(r[name]) for r in rows if name in r and not math.isnan(float(r[name]))]
        out[name] = sum(vals) / len(vals) if vals else float("nan")
    return out


def _field(v) -> str:
    return "" if isinstance(v, float) and math.isnan(v) else repr(float(v))


def eval_dataset(args, tapvid_fn: Optional[Callable] = None, badja_fn: Optional[Callable] = None) -> Dict[str, float]:
    """eval/eval_benchmark.py:9-44.  `tapvid_fn(trajectories_dir, occlusions_dir, video_config, pred_video_sizes)` and
    `badja_fn(trajectories_dir, video_config, pred_video_sizes)` default to the device scorers above.  Returns the means."""
    if args.dataset_type not in ("tapvid", "BADJA"):
        raise ValueError("Invalid dataset type. Must be either tapvid or BADJA")
    tapvid_fn = tapvid_fn or tapvid_video_metrics
    badja_fn = badja_fn or badja_video_metrics
    with open(args.benchmark_pickle_path, "rb") as fh:
        benchmark_data = pickle.load(fh)
    sizes = list(args.pred_video_sizes)
    rows, names = [], []
    for video_idx_str in os.listdir(args.dataset_root_dir):
        if video_idx_str.startswith("."):
            continue
        video_dir = os.path.join(args.dataset_root_dir, video_idx_str)
        video_idx = int(video_idx_str)
        config = get_video_config_by_video_id(benchmark_data, video_idx)
        if args.dataset_type == "tapvid":
            metrics = dict(tapvid_fn(os.path.join(video_dir, "trajectories"), os.path.join(video_dir, "occlusions"), config, sizes))
        else:
            metrics = dict(badja_fn(os.path.join(video_dir, "trajectories"), config, sizes))
        for name in metrics:   # the order of the reference's dict, first seen first
            if name not in names:
                names.append(name)
        rows.append((video_idx, metrics))
    means = column_means([m for _, m in rows], names)
    out_dir = os.path.dirname(args.out_file)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out_file, "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(["video_idx"] + names)
        for video_idx, m in rows:
            w.writerow([video_idx] + [_field(m.get(n, float("nan"))) for n in names])
        w.writerow(["average"] + [_field(means[n]) for n in names])
    print("Total metrics:")
    for n in names:
        print(f"{n:<28}{means[n]:.6f}")
    return means


def make_parser() -> argparse.ArgumentParser:
    """eval_benchmark.py:46-52, plus --pred-video-sizes (hard-coded to [854, 476] there)."""
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--dataset-root-dir", default="./dataset/davis_256", type=str)
    p.add_argument("--benchmark-pickle-path", default="./dataset/davis.pkl", type=str, help="the benchmark file; it is unpickled")
    p.add_argument("--out-file", default="./tapvid/comp_metrics.csv", type=str)
    p.add_argument("--dataset-type", default="tapvid", type=str, help="Dataset type: tapvid or BADJA")
    p.add_argument("--pred-video-sizes", type=int, nargs=2, default=(854, 476), metavar=("W", "H"),
                   help="raster of the saved predictions, (w, h)")
    return p


if __name__ == "__main__":
    eval_dataset(make_parser().parse_args())
