"""Times the optical-flow preprocessing on one GPU at T = 90 frames of 476 x 854 (token grid 67 x 121 at stride 7): fg / bg
split, nearest trajectory per grid point, optical-flow filter of the best buddies (1000 per frame pair) --
against the ATen restatement in the reference's 30-row batching (of_filter_dino_best_buddies.get_closest_traj_idx_batch).

    python scripts/of_prep_time.py [--sizes 1000000 2000000 3000000] [--out FILE.json]

The nearest search's share of the fp32 vector peak counts 5 flops per (grid point, tracked candidate) pair (2 sub, 2 mul, 1 add)
against 157.3 TFLOP/s.  The ATen search is timed on `--aten-frames` frames and scaled to 90 (it is linear in the frames).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dino_tracker_amd import ops  # noqa: E402
from dino_tracker_amd.best_buddies import create_meshgrid  # noqa: E402
from dino_tracker_amd.of_preprocessing import ORIGIN, grid_dims, of_filter_best_buddies, split_trajectories_fg_bg  # noqa: E402

DEV = "cuda:0"
PEAK_FP32 = 157.3e12
T, H, W = 90, 476, 854


def synth(N, seed=5):
    """RAFT-like trajectories [N, T, 2]: integer start pixel at a random frame, a smooth per-frame flow, a random end."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    s0 = torch.randint(0, T - 1, (N,), generator=g, device=DEV)
    length = 2 + (torch.rand(N, generator=g, device=DEV) * (T - s0 - 1).float()).long()
    end = torch.minimum(s0 + length - 1, torch.tensor(T - 1, device=DEV))
    p = torch.stack([torch.randint(0, W, (N,), generator=g, device=DEV), torch.randint(0, H, (N,), generator=g, device=DEV)], 1).float()
    coef = (torch.rand((T, 2, 3), generator=g, device=DEV) - 0.5) * 6
    traj = torch.full((N, T, 2), float("nan"), device=DEV)
    for t in range(T):
        live = (t >= s0) & (t <= end)
        traj[:, t] = torch.where(live[:, None], p, traj[:, t])
        c = coef[t]
        p = torch.where((t >= s0)[:, None], p + c[:, 0] + c[:, 1] * p[:, :1] / W + c[:, 2] * p[:, 1:] / H, p)
    return traj


def synth_bb(per=1000, seed=9):
    g = torch.Generator(device=DEV).manual_seed(seed)
    grid = create_meshgrid(H, W, 7, 14, DEV)
    bb = {}
    for s in range(T):
        for t in range(T):
            if s != t:
                i = torch.randint(0, grid.shape[0], (2, per), generator=g, device=DEV)
                bb[f"{s}_{t}"] = {"source_coords": grid[i[0]], "target_coords": grid[i[1]],
                                  "cos_sims": torch.rand(per, generator=g, device=DEV)}
    return bb


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def aten_nearest(traj, grid, frames, batch=30):
    for t in frames:
        pts = traj[:, t]
        for i in range(0, grid.shape[0], batch):
            d = torch.norm(pts[None] - grid[i:i + batch, None], dim=2)
            torch.nan_to_num(d, nan=torch.inf).argmin(dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 2_000_000, 3_000_000])
    ap.add_argument("--aten-frames", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "of_prep_time.py measures on a GPU"
    gh, gw = grid_dims(H, W)
    grid = create_meshgrid(H, W, 7, 14, DEV)
    masks = (torch.rand((T, H, W), generator=torch.Generator(device=DEV).manual_seed(1), device=DEV) < 0.3).to(torch.uint8) * 255
    bb = synth_bb()
    rows = []
    for N in a.sizes:
        traj = synth(N)
        tracked = int((~traj.isnan().any(-1)).sum())
        t_split, _ = timed(lambda: split_trajectories_fg_bg(traj, masks, DEV))
        t_nn, idx = timed(lambda: ops.nearest_traj(traj, gh, gw, ORIGIN, 7))
        t_filter, _ = timed(lambda: of_filter_best_buddies(bb, traj, H, W, 7, DEV, idx=idx))
        pairs = gh * gw * tracked
        frames = list(range(0, T, max(1, T // a.aten_frames)))[:a.aten_frames]
        t0 = time.perf_counter()
        aten_nearest(traj, grid, frames)
        torch.cuda.synchronize()
        t_aten = (time.perf_counter() - t0) * T / len(frames)
        row = {"N": N, "T": T, "grid": [gh, gw], "tracked_points": tracked, "split_ms": 1e3 * t_split,
               "nearest_ms": 1e3 * t_nn, "filter_ms": 1e3 * t_filter, "filter_buddies": 1000 * T * (T - 1),
               "total_ms": 1e3 * (t_split + t_nn + t_filter),
               "nearest_pairs": pairs, "nearest_fp32_peak_frac": 5 * pairs / t_nn / PEAK_FP32,
               "aten_nearest_30row_ms_extrapolated": 1e3 * t_aten, "aten_frames_timed": len(frames)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del traj, idx
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
