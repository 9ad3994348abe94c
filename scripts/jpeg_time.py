"""Video output on one MI355X (docs/MEASUREMENTS.md, "Video output"):
    python scripts/jpeg_time.py [out.json]
save_video(container="avi") against the PNG fallback (container=None without imageio) on the same rendered frames, wall clock and
synchronised, alternating, after a warm-up; where the avi path spends its time (encode to the read-back, download, file write);
the kernel times of the three stages from the dtk_profile_* hooks; file sizes; PSNR of the decoded frames against the rendered ones.
The frames are synth.synth_video (a panning box-filtered random colour texture with noise) with 300 dotted tracks rendered on it."""
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from PIL import Image  # noqa: E402

from dino_tracker_amd import ops, synth, video_out, visualize as V  # noqa: E402

out = {}
tmp = tempfile.mkdtemp()
for name, (T, H, W, runs) in (("854x480", (90, 480, 854, 5)), ("1920x1080", (30, 1080, 1920, 3))):
    torch.manual_seed(0)
    base = (synth.synth_video(T, H, W, seed=3) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()
    rng = np.random.default_rng(0)
    N = 300
    start = rng.uniform([0, 0], [W, H], (N, 2))
    pts = (start[:, None] + np.arange(T)[None, :, None] * rng.normal(0, 1.5, (N, 1, 2))).astype(np.float32)
    occ = (rng.random((N, T)) < 0.1).astype(np.int32)
    video = V.plot_tracks_v2(base, pts, occ, rainbow_colors=True, point_size=40)
    torch.cuda.synchronize()
    r = {"frames": T, "raw_bytes": int(video.numel())}
    path = os.path.join(tmp, name + ".mp4")
    V.save_video(video, path, fps=10, container="avi")          # warm
    times = {"avi": [], "png": []}
    for i in range(runs):
        for how in ("avi", "png"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w = V.save_video(video, path, fps=10, container="avi" if how == "avi" else None)
            torch.cuda.synchronize()
            times[how].append(time.perf_counter() - t0)
            if how == "png":
                r["png_bytes"] = sum(os.path.getsize(os.path.join(w, f)) for f in os.listdir(w))
                shutil.rmtree(w)
            else:
                r["avi_bytes"] = os.path.getsize(w)
    r["save_video_s"] = times
    # where the avi path spends its time: encode (device, to the read-back), download, file
    parts = {"encode_s": [], "download_s": [], "write_s": []}
    for i in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data, offsets = video_out.encode_jpeg(video, 90)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host = data.cpu().numpy().tobytes()
        t2 = time.perf_counter()
        with open(os.path.join(tmp, "raw.bin"), "wb") as fh:
            fh.write(host)
        t3 = time.perf_counter()
        parts["encode_s"].append(t1 - t0), parts["download_s"].append(t2 - t1), parts["write_s"].append(t3 - t2)
    r["parts"] = parts
    ops.profile_enable(True)
    for i in range(3):
        video_out.encode_jpeg(video, 90)
    prof = ops.profile_collect()
    ops.profile_enable(False)
    r["kernel_ms_per_encode_of_all_frames"] = {k: [v[0] / 3, v[1] // 3] for k, v in prof.items() if k.startswith("jpeg")}
    frames = video_out.read_mjpeg_avi(os.path.join(tmp, name + ".avi"))
    host = video.cpu().numpy()
    psnr = []
    for data, ref in zip(frames, host):
        dec = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).astype(np.float64)
        psnr.append(10 * np.log10(255.0 ** 2 / np.mean((dec - ref) ** 2)))
    r["psnr_db"] = [float(np.min(psnr)), float(np.mean(psnr)), float(np.max(psnr))]
    r["batches"] = -(-T // video_out.frames_per_batch(T, H, W))
    out[name] = r
    print(name, json.dumps(r), flush=True)
    del video, base
    torch.cuda.empty_cache()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
shutil.rmtree(tmp)
