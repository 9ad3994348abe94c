"""PNG output on one MI355X (docs/MEASUREMENTS.md, "PNG encode"):
    python scripts/png_encode_time.py [out.json]
save_video(container="png") -- the device encoder -- against the PNG fallback (container=None without imageio: Pillow on one host
thread) on the frames of scripts/jpeg_time.py, wall clock and synchronised, alternating, five runs each after a warm-up; where the
device path spends its time (encode to the read-back, download, file writes); the kernel times from the dtk_profile_* hooks; the bytes
written against Pillow's default and against zlib level 1 on the same filtered rows."""
import io
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from PIL import Image  # noqa: E402

from dino_tracker_amd import ops, png_out, synth, visualize as V  # noqa: E402

out = {}
tmp = tempfile.mkdtemp()
RUNS = 5
for name, (T, H, W) in (("854x480", (90, 480, 854)), ("1920x1080", (30, 1080, 1920))):
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
    shutil.rmtree(V.save_video(video, path, fps=10, container="png"))          # warm
    times = {"device": [], "host": []}
    for i in range(RUNS):
        for how in ("device", "host"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w = V.save_video(video, path, fps=10, container="png" if how == "device" else None)
            torch.cuda.synchronize()
            times[how].append(time.perf_counter() - t0)
            r[how + "_bytes"] = sum(os.path.getsize(os.path.join(w, f)) for f in os.listdir(w))
            if i == 0 and how == "device":                                      # what was written is the video
                got = np.stack([np.asarray(Image.open(os.path.join(w, f))) for f in sorted(os.listdir(w))[:3]])
                assert np.array_equal(got, video[:3].cpu().numpy())
            shutil.rmtree(w)
    r["save_video_s"] = times
    parts = {"encode_s": [], "download_s": [], "write_s": []}
    for i in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data, offsets = png_out.encode_png(video)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host, offs = data.cpu().numpy().tobytes(), offsets.cpu().tolist()
        t2 = time.perf_counter()
        os.makedirs(os.path.join(tmp, "w"), exist_ok=True)
        for k, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
            with open(os.path.join(tmp, "w", f"{k:05d}.png"), "wb") as fh:
                fh.write(host[a:b])
        t3 = time.perf_counter()
        parts["encode_s"].append(t1 - t0), parts["download_s"].append(t2 - t1), parts["write_s"].append(t3 - t2)
    r["parts"] = parts
    ops.profile_enable(True)
    for i in range(3):
        png_out.encode_png(video)
    prof = ops.profile_collect()
    ops.profile_enable(False)
    r["kernel_ms_per_encode_of_all_frames"] = {k: [v[0] / 3, v[1] // 3] for k, v in prof.items()
                                               if k.startswith(("png", "deflate", "crc"))}
    # the bytes: ours, Pillow's default, zlib level 1 and 6 on the rows our filter stage made (the first 8 frames)
    K = 8
    raw = ops.png_filter(video[:K]).cpu().numpy()
    ours = [b - a for a, b in zip(offs[:K], offs[1:K + 1])]
    pil = []
    for f in range(K):
        buf = io.BytesIO()
        Image.fromarray(video[f].cpu().numpy()).save(buf, format="PNG")
        pil.append(len(buf.getvalue()))
    r["bytes_first_frames"] = {"frames": K, "raw_rows": int(raw[0].size) * K, "device": int(sum(ours)), "pillow_default": int(sum(pil)),
                               "zlib1_same_rows": int(sum(len(zlib.compress(raw[f].tobytes(), 1)) + 57 for f in range(K))),
                               "zlib6_same_rows": int(sum(len(zlib.compress(raw[f].tobytes(), 6)) + 57 for f in range(K)))}
    r["batches"] = -(-T // png_out.frames_per_batch(T, H, W, 3))
    out[name] = r
    print(name, json.dumps(r), flush=True)
    del video, base
    torch.cuda.empty_cache()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
shutil.rmtree(tmp)
