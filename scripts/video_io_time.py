"""Timings of the device video ingest (docs/MEASUREMENTS.md): 90 frames, (a) 854 x 480 -> 854 x 476 and (b) 1920 x 1080 -> 854 x 476.
    python scripts/video_io_time.py [out.json] [--frames 90] [--repeats 5] [--no-folder]
Kernel time: device events around video_io.resize_lanczos (uint8 frames on the device -> fp32 [T, 3, h, w]) after a warm-up, in the
form the entry point picks and in the forced general form, beside the floor: a plain device copy that moves the same number of bytes
(input bytes read + output bytes written).
Whole load_video: wall clock (synchronised) of video_io.load_video on a folder of PNG frames against the host path followed by its
upload, train.load_video(...).to(device) -- the code every caller ran before the device path existed -- `repeats` times each, with the
host path's own run-to-run spread."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dino_tracker_amd import train, video_io  # noqa: E402

DEV = "cuda:0"
SHAPES = {"854x480_to_854x476": (480, 854, 476, 854), "1920x1080_to_854x476": (1080, 1920, 476, 854)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def scene(T, H, W, seed):
    """A panning smooth pattern plus mild noise: compresses like footage rather than like white noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = 127.5 + 60 * np.stack([np.sin(xx / 37.0) + np.cos(yy / 23.0), np.sin((xx - yy) / 51.0), np.cos((xx + yy) / 67.0)], -1)
    frames = np.empty((T, H, W, 3), dtype=np.uint8)
    for t in range(T):
        noise = rng.integers(-6, 7, size=(H, W, 3), dtype=np.int16)
        frames[t] = np.clip(np.roll(base, 3 * t, axis=1) + noise, 0, 255).astype(np.uint8)
    return frames


def kernel_times(frames, h, w, repeats):
    x = torch.from_numpy(frames).to(DEV)
    out = {}
    for name, general in (("picked_form_ms", False), ("general_form_ms", True)):
        video_io.resize_lanczos(x, h, w, out="f32", force_general=general)   # warm-up: tables, allocator
        torch.cuda.synchronize()
        out[name] = [event_ms(lambda: video_io.resize_lanczos(x, h, w, out="f32", force_general=general)) for _ in range(repeats)]
    in_bytes, out_bytes = x.numel(), x.shape[0] * 3 * h * w * 4
    a = torch.empty((in_bytes + out_bytes) // 2, dtype=torch.uint8, device=DEV)
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    out["copy_floor_ms"] = [event_ms(lambda: b.copy_(a)) for _ in range(repeats)]
    out["bytes_in"], out["bytes_out"] = in_bytes, out_bytes
    return out


def folder_times(frames, h, w, repeats):
    from PIL import Image
    with tempfile.TemporaryDirectory() as folder:
        for t, f in enumerate(frames):
            Image.fromarray(f).save(os.path.join(folder, f"{t:05d}.png"), compress_level=1)
        host = [wall_ms(lambda: train.load_video(folder, resize=(h, w)).to(DEV)) for _ in range(repeats)]
        video_io.load_video(folder, resize=(h, w), num_frames=2, device=DEV)   # warm-up: tables, pinned allocator
        dev = [wall_ms(lambda: video_io.load_video(folder, resize=(h, w), device=DEV)) for _ in range(repeats)]
        same = torch.equal(video_io.load_video(folder, resize=(h, w), device=DEV).cpu(), train.load_video(folder, resize=(h, w)))
    return {"host_load_video_to_device_ms": host, "device_load_video_ms": dev, "host_spread_ms": max(host) - min(host),
            "bit_equal": same}


def main():
    args = sys.argv[1:]
    T = int(args[args.index("--frames") + 1]) if "--frames" in args else 90
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 5
    out = {"frames": T, "repeats": repeats}
    for name, (H, W, h, w) in SHAPES.items():
        frames = scene(T, H, W, seed=H)
        out[name] = {"kernel": kernel_times(frames, h, w, repeats)}
        if "--no-folder" not in args:
            out[name]["load_video"] = folder_times(frames, h, w, repeats)
        print(json.dumps({name: out[name]}), flush=True)
    if args and not args[0].startswith("--"):
        with open(args[0], "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
