"""Timings of the track-video rasteriser (docs/MEASUREMENTS.md): a 90-frame 854 x 476 trail video with 4 000 points
(16.4 M primitives), per stage and per video, beside the floor of reading and writing the frames once.
    python scripts/render_time.py [out.json]
Video time: device events around plot_tracks_tails on device tensors, after a warm-up (it includes the per-group read-back of the
key count and torch's cumsum / sort / searchsorted).  Stage times: the library's own per-launch events for the four kernels, and
device events around the torch calls, in a pass of their own over the same frame groups."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dino_tracker_amd import ops, visualize as V  # noqa: E402

DEV = "cuda:0"
T, H, W, N = 90, 476, 854, 4000
POINT_SIZE, LINEWIDTH = 40, 1.5


def scene():
    """A pan of 3 px / frame with mild perspective; points on a jittered grid over a moving object region, 10 % occluded."""
    rng = np.random.default_rng(0)
    homogs = np.stack([np.array([[1 + 1e-3 * t, 2e-4 * t, -3.0 * t], [-1e-4 * t, 1 + 1e-3 * t, -0.8 * t], [2e-6 * t, -1e-6 * t, 1.0]])
                       for t in range(T)])
    homogs = np.stack([np.linalg.inv(h) for h in homogs])          # frame -> canonical
    start = rng.uniform([250, 120], [600, 380], size=(N, 2))
    vel = np.array([1.5, 0.4]) + rng.normal(0, 0.15, size=(N, 2))
    t = np.arange(T)[None, :, None]
    pts = start[:, None] + vel[:, None] * t + 6 * np.sin(t / 7.0 + start[:, None, :1] / 40.0)
    occ = rng.random((N, T)) < 0.10
    video = rng.integers(0, 256, size=(T, H, W, 3), dtype=np.uint8)
    return video, pts.astype(np.float32), occ, homogs


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def main():
    video, pts, occ, homogs = scene()
    v, p, o = torch.from_numpy(video).to(DEV), torch.from_numpy(pts).to(DEV), torch.from_numpy(occ).to(DEV)
    kw = dict(point_size=POINT_SIZE, linewidth=LINEWIDTH, marker="D")
    out = {"T": T, "H": H, "W": W, "N": N}
    stats = {}
    V.plot_tracks_tails(v, p, o, homogs, stats=stats, **kw)                     # warm-up
    torch.cuda.synchronize()
    out.update(stats)
    out["video_ms"] = [event_ms(lambda: V.plot_tracks_tails(v, p, o, homogs, **kw))[0] for _ in range(3)]
    out["dotted_video_ms"] = [event_ms(lambda: V.plot_tracks_v2(v, p, o, rainbow_colors=True, point_size=POINT_SIZE))[0]
                              for _ in range(3)]
    out["floor_ms_frames_once_6.3TBs"] = 2 * video.size / 6.3e12 * 1e3

    # per stage, over the same frame groups
    groups = V.frame_groups(ops.RENDER_TAILS, N, T, H, W)
    colors = torch.from_numpy(V.rainbow_colors(N)).to(DEV).float()
    maps = torch.from_numpy(V.frame_maps(homogs)).to(DEV)
    o8 = o.to(torch.uint8)
    stage = {k: 0.0 for k in ("cumsum_ms", "readback_ms", "sort_ms", "searchsorted_ms")}
    ops.profile_enable(True)
    for f0, F in groups:
        rec = ops.render_prims(p, o8, colors, maps, f0, F, H, W, ops.RENDER_TAILS, ops.RENDER_DIAMOND, V.marker_size("D", POINT_SIZE),
                               LINEWIDTH * V.PX_PER_POINT / 2)
        counts = ops.render_tile_counts(rec, F, H, W)
        ms, ends = event_ms(lambda: torch.cumsum(counts, 0, dtype=torch.int64))
        stage["cumsum_ms"] += ms
        ms, K = event_ms(lambda: int(ends[-1].item()))
        stage["readback_ms"] += ms
        keys = ops.render_tile_keys(rec, (ends - counts).contiguous(), K, F, H, W)
        ms, srt = event_ms(lambda: torch.sort(keys).values)
        stage["sort_ms"] += ms
        ms, starts = event_ms(lambda: ops.render_tile_starts(srt, F, H, W))
        stage["searchsorted_ms"] += ms
        ops.render_blend(v[f0:f0 + F], rec, srt, starts)
        out.setdefault("group_bytes", []).append(ops.render_group_bytes(len(rec), K, F, H, W))
        out.setdefault("group_keys_per_prim", []).append(K / len(rec))
    prof = ops.profile_collect()
    ops.profile_enable(False)
    out["groups"] = groups
    out["kernels_ms_per_video"] = {k: v[0] for k, v in prof.items() if k.startswith("render_")}
    out["kernel_launches"] = {k: v[1] for k, v in prof.items() if k.startswith("render_")}
    out["torch_ms_per_video"] = stage
    print(json.dumps(out), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
