"""Timings of the device JPEG decoder (docs/MEASUREMENTS.md, "JPEG decode"): 90 frames of 854 x 480 and of 1920 x 1080 from
synth.synth_video, written at quality 90 (a) by Pillow with its defaults -- no restart markers: ONE segment per frame -- and (b) by
video_out.write_jpeg_frames -- a restart interval of 16 MCUs: 102 and 510 segments per frame.
    python scripts/jpeg_decode_time.py [out.json] [--frames 90] [--frames-1080 N] [--repeats 7] [--sampling 420|422|444|gray]
--sampling other than 420 ("JPEG decode: other samplings"): both folders are Pillow's, (a) with its defaults and (b) with
restart_marker_blocks=16 -- the same interval of 16 MCUs, which are smaller there -- and gray frames are the video's green channel.
--frames-1080: the frame count of the 1920 x 1080 video (default: --frames).
Stages: device events around ops.jpeg_decode_coefficients (bytes already on the device) and ops.jpeg_pixels, after a warm-up.
Whole load_video: wall clock (synchronised), warm file cache, DTK_JPEG_DECODE=host -- the code load_video ran before the decoder
existed: Pillow into one pinned buffer, one upload, the resize -- against DTK_JPEG_DECODE=device, alternating, `repeats` times each,
with the host path's own run-to-run spread.  The two results are compared with torch.equal."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dino_tracker_amd import ops, synth, video_in, video_io, video_out  # noqa: E402

DEV = "cuda:0"
SHAPES = {"854x480": (480, 854), "1920x1080": (1080, 1920)}
RESIZE = (476, 854)


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


def load(folder, mode):
    os.environ["DTK_JPEG_DECODE"] = mode
    try:
        return video_io.load_video(folder, resize=RESIZE, device=DEV)
    finally:
        del os.environ["DTK_JPEG_DECODE"]


def measure(folder, repeats):
    files = video_io.video_files(folder)
    pinned, views = video_in.read_pinned(files)
    plan, why = video_in.plan_jpeg_sampled(views)
    assert plan is not None, why
    stream = pinned.to(DEV)
    huff, qt = torch.from_numpy(plan.huffman).to(DEV), torch.from_numpy(plan.qtables).to(DEV)
    H, W, S = plan.height, plan.width, plan.sampling
    coef, status = ops.jpeg_decode_coefficients(stream, plan.segments, huff, H, W, S)   # warm-up
    ops.jpeg_pixels(coef, qt, H, W, sampling=S)
    assert not bool(status.any())
    out = {"sampling": video_in.SAMPLING_NAMES[S], "frames": plan.frames, "bytes": int(stream.numel()),
           "segments_per_frame": plan.segments.shape[0] // plan.frames,
           "entropy_ms": [event_ms(lambda: ops.jpeg_decode_coefficients(stream, plan.segments, huff, H, W, S)) for _ in range(repeats)],
           "pixels_ms": [event_ms(lambda: ops.jpeg_pixels(coef, qt, H, W, sampling=S)) for _ in range(repeats)]}
    t0 = time.perf_counter()
    video_in.plan_jpeg_sampled(video_in.read_pinned(files)[1])
    out["read_and_parse_ms"] = (time.perf_counter() - t0) * 1e3
    load(folder, "host"), load(folder, "device")                                                          # warm-up
    host, dev = [], []
    for _ in range(repeats):
        host.append(wall_ms(lambda: load(folder, "host")))
        dev.append(wall_ms(lambda: load(folder, "device")))
    out.update(host_load_video_ms=host, device_load_video_ms=dev, host_spread_ms=max(host) - min(host),
               host_median_ms=float(np.median(host)), device_median_ms=float(np.median(dev)),
               bit_equal=torch.equal(load(folder, "host"), load(folder, "device")))
    return out


def main():
    from PIL import Image
    args = sys.argv[1:]
    T = int(args[args.index("--frames") + 1]) if "--frames" in args else 90
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 7
    T1080 = int(args[args.index("--frames-1080") + 1]) if "--frames-1080" in args else T
    sampling = args[args.index("--sampling") + 1] if "--sampling" in args else "420"
    if sampling not in ("420", "422", "444", "gray"):
        raise SystemExit(f"--sampling must be 420, 422, 444 or gray, got {sampling!r}")
    kw = {"420": {}, "422": {"subsampling": 1}, "444": {"subsampling": 0}, "gray": {}}[sampling]
    out = {"frames": T, "frames_1080": T1080, "repeats": repeats, "sampling": sampling}
    for name, (H, W) in SHAPES.items():
        n = T1080 if name == "1920x1080" else T
        frames = synth.synth_video(n, H, W, seed=H).mul(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        with tempfile.TemporaryDirectory() as root:
            plain, own = os.path.join(root, "pillow"), os.path.join(root, "dri16")
            os.makedirs(plain)
            for t, f in enumerate(frames.numpy()):
                Image.fromarray(f[..., 1] if sampling == "gray" else f).save(os.path.join(plain, f"{t:05d}.jpg"), quality=90, **kw)
            if sampling == "420":
                video_out.write_jpeg_frames(frames.to(DEV), own, quality=90)
            else:
                os.makedirs(own)
                for t, f in enumerate(frames.numpy()):
                    Image.fromarray(f[..., 1] if sampling == "gray" else f).save(os.path.join(own, f"{t:05d}.jpg"), quality=90,
                                                                                 restart_marker_blocks=16, **kw)
            out[name] = {"no_restart": measure(plain, repeats), "restart_16": measure(own, repeats)}
        print(json.dumps({name: out[name]}), flush=True)
    for name in SHAPES:          # the bar of video_io.JPEG_AUTO_SAMPLINGS: not slower than the host path beyond its own spread
        for kind, m in out[name].items():
            m["device_within_host_spread"] = m["device_median_ms"] <= m["host_median_ms"] + m["host_spread_ms"]
    print(json.dumps({"meets_the_bar": all(m["device_within_host_spread"] for name in SHAPES for m in out[name].values())}), flush=True)
    if args and not args[0].startswith("--"):
        with open(args[0], "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
