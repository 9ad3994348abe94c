"""Timings of the device PNG decoder (docs/MEASUREMENTS.md "PNG decode"): the synthetic panning frames of scripts/video_io_time.py,
90 frames of 854 x 480 and 30 of 1920 x 1080, written by Pillow at compress_level 1 and 6.
    python scripts/png_decode_time.py [out.json] [--frames-small 90] [--frames-large 30] [--repeats 5]
Whole load_video: wall clock (synchronised) of video_io.load_video with DTK_PNG_DECODE=host against DTK_PNG_DECODE=device, in this
process, alternating, `repeats` times each after a warm-up of both, with the host path's own spread (max - min): `auto` may select the
device only where device <= host + spread everywhere.
Kernels: device events around dtk_inflate, dtk_adler32 and dtk_png_unfilter on the uploaded streams, with the compressed and raw byte
counts and the rates per wave they imply (one wave per frame, all of them resident for the whole launch)."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dino_tracker_amd import ops, png_in, video_io  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_io_time import event_ms, scene, wall_ms  # noqa: E402

DEV = "cuda:0"
SHAPES = {"854x480_to_854x476": (480, 854, 476, 854, "--frames-small", 90), "1920x1080_to_854x476": (1080, 1920, 476, 854, "--frames-large", 30)}


def load(folder, h, w, mode):
    os.environ["DTK_PNG_DECODE"] = mode
    return video_io.load_video(folder, resize=(h, w), device=DEV)


def kernel_times(files, repeats):
    pinned, plan, datas, why = png_in.read_pinned(files)
    assert plan is not None, why
    stream = pinned.to(DEV)
    raw_bytes = plan.frames * plan.headers[0].raw_bytes
    out = {"compressed_bytes": int(plan.streams[:, 1].sum()), "raw_bytes": int(raw_bytes), "frames": plan.frames}
    raw, status = ops.inflate(stream, plan.streams, raw_bytes)      # warm-up
    ops.adler32(stream, plan.streams, raw, status)
    ops.png_unfilter(raw, plan.frames, plan.height, plan.width, plan.bpp, status)
    assert not bool(status.any().item())
    out["inflate_ms"] = [event_ms(lambda: ops.inflate(stream, plan.streams, raw_bytes)) for _ in range(repeats)]
    out["adler32_ms"] = [event_ms(lambda: ops.adler32(stream, plan.streams, raw, status)) for _ in range(repeats)]
    out["png_unfilter_ms"] = [event_ms(lambda: ops.png_unfilter(raw, plan.frames, plan.height, plan.width, plan.bpp, status))
                              for _ in range(repeats)]
    ms = min(out["inflate_ms"])
    out["raw_MB_per_s_per_wave"] = raw_bytes / plan.frames / (ms * 1e-3) / 1e6       # every wave works for the whole launch
    out["compressed_Mbit_per_s_per_wave"] = 8 * out["compressed_bytes"] / plan.frames / (ms * 1e-3) / 1e6
    return out


def folder_times(frames, h, w, level, repeats):
    from PIL import Image
    with tempfile.TemporaryDirectory() as folder:
        for t, f in enumerate(frames):
            Image.fromarray(f).save(os.path.join(folder, f"{t:05d}.png"), compress_level=level)
        files = video_io.video_files(folder)
        host0, dev0 = load(folder, h, w, "host"), load(folder, h, w, "device")      # warm-up of both, and the equality
        same = torch.equal(host0, dev0)
        del host0, dev0
        host, dev = [], []
        for _ in range(repeats):
            host.append(wall_ms(lambda: load(folder, h, w, "host")))
            dev.append(wall_ms(lambda: load(folder, h, w, "device")))
        t0 = time.perf_counter()
        png_in.read_pinned(files)
        read_ms = (time.perf_counter() - t0) * 1e3
        kern = kernel_times(files, repeats)
    spread = max(host) - min(host)
    return {"host_ms": host, "device_ms": dev, "host_spread_ms": spread, "bit_equal": same, "read_and_plan_ms": read_ms,
            "device_not_slower": bool(np.median(dev) <= np.median(host) + spread), "kernels": kern}


def main():
    args = sys.argv[1:]
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 5
    out = {"repeats": repeats}
    for name, (H, W, h, w, flag, default) in SHAPES.items():
        T = int(args[args.index(flag) + 1]) if flag in args else default
        frames = scene(T, H, W, seed=H)
        for level in (1, 6):
            out[f"{name}_level{level}"] = folder_times(frames, h, w, level, repeats)
            print(json.dumps({f"{name}_level{level}": out[f"{name}_level{level}"]}), flush=True)
    out["auto_may_use_device"] = all(v["device_not_slower"] for k, v in out.items() if isinstance(v, dict))
    print(json.dumps({"auto_may_use_device": out["auto_may_use_device"]}), flush=True)
    if args and not args[0].startswith("--"):
        with open(args[0], "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
