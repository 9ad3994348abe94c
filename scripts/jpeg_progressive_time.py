"""Timings of the device decoder of PROGRESSIVE JPEG files (docs/MEASUREMENTS.md, "JPEG decode: progressive"): the frames of
scripts/jpeg_decode_time.py -- synth.synth_video, 854 x 480 and 1920 x 1080, 4:2:0, quality 90 -- written by Pillow with
progressive=True (a) without restart markers, what real files have: every scan is ONE segment, and (b) with
restart_marker_blocks=16.
    python scripts/jpeg_progressive_time.py [out.json] [--frames 90] [--frames-1080 30] [--repeats 7]
Stage: device events around ops.jpeg_decode_progressive (bytes already on the device; the launches of all levels) and
ops.jpeg_pixels, after a warm-up.  Whole load_video: wall clock (synchronised), warm file cache, DTK_JPEG_DECODE=host -- Pillow into
one pinned buffer, one upload, the resize -- against DTK_JPEG_DECODE=device, alternating, `repeats` times each, with the host path's
own run-to-run spread.  The two results are compared with torch.equal."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dino_tracker_amd import ops, synth, video_in, video_io  # noqa: E402
from jpeg_decode_time import DEV, SHAPES, event_ms, load, wall_ms  # noqa: E402


def measure(folder, repeats):
    files = video_io.video_files(folder)
    pinned, views = video_in.read_pinned(files)
    plan, why = video_in.plan_jpeg_progressive(views)
    assert plan is not None, why
    stream = pinned.to(DEV)
    tables, qt = torch.from_numpy(plan.tables).to(DEV), torch.from_numpy(plan.qtables).to(DEV)
    F, H, W, S = plan.frames, plan.height, plan.width, plan.sampling

    def entropy():
        return ops.jpeg_decode_progressive(stream, plan.segments, tables, F, H, W, S)
    coef, status = entropy()                                                                             # warm-up
    ops.jpeg_pixels(coef, qt, H, W, sampling=S)
    assert not bool(status.any())
    levels = plan.segments[:, 3]
    out = {"frames": F, "bytes": int(stream.numel()), "segments_per_frame": plan.segments.shape[0] // F,
           "segments_per_level_per_frame": [int((levels == lv).sum()) // F for lv in range(int(levels.max()) + 1)],
           "longest_segment_bytes": int(plan.segments[:, 2].max()),
           "entropy_ms": [event_ms(entropy) for _ in range(repeats)],
           "pixels_ms": [event_ms(lambda: ops.jpeg_pixels(coef, qt, H, W, sampling=S)) for _ in range(repeats)]}
    t0 = time.perf_counter()
    video_in.plan_jpeg_progressive(video_in.read_pinned(files)[1])
    out["read_and_parse_ms"] = (time.perf_counter() - t0) * 1e3
    load(folder, "host"), load(folder, "device")                                                          # warm-up
    host, dev = [], []
    for _ in range(repeats):
        host.append(wall_ms(lambda: load(folder, "host")))
        dev.append(wall_ms(lambda: load(folder, "device")))
    out.update(host_load_video_ms=host, device_load_video_ms=dev, host_spread_ms=max(host) - min(host),
               host_median_ms=float(np.median(host)), device_median_ms=float(np.median(dev)),
               bit_equal=torch.equal(load(folder, "host"), load(folder, "device")))
    out["device_within_host_spread"] = out["device_median_ms"] <= out["host_median_ms"] + out["host_spread_ms"]
    return out


def main():
    from PIL import Image, ImageFile
    args = sys.argv[1:]
    T = int(args[args.index("--frames") + 1]) if "--frames" in args else 90
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 7
    T1080 = int(args[args.index("--frames-1080") + 1]) if "--frames-1080" in args else 30
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 1 << 24)      # a progressive file is written from one buffer
    out = {"frames": T, "frames_1080": T1080, "repeats": repeats}
    for name, (H, W) in SHAPES.items():
        n = T1080 if name == "1920x1080" else T
        frames = synth.synth_video(n, H, W, seed=H).mul(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        with tempfile.TemporaryDirectory() as root:
            out[name] = {}
            for kind, kw in (("no_restart", {}), ("restart_16", {"restart_marker_blocks": 16})):
                folder = os.path.join(root, kind)
                os.makedirs(folder)
                for t, f in enumerate(frames.numpy()):
                    Image.fromarray(f).save(os.path.join(folder, f"{t:05d}.jpg"), quality=90, progressive=True, **kw)
                out[name][kind] = measure(folder, repeats)
        print(json.dumps({name: out[name]}), flush=True)
    print(json.dumps({"meets_the_bar": all(m["device_within_host_spread"] for name in SHAPES for m in out[name].values())}), flush=True)
    if args and not args[0].startswith("--"):
        with open(args[0], "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
