"""Timings of the parallel JPEG entropy stage (docs/MEASUREMENTS.md, "JPEG decode: parallel entropy stage") against the sequential
one, on the same tree and the same GPU in one run:
    python scripts/jpeg_parallel_time.py [out.json] [--frames 90] [--frames-1080 30] [--repeats 7] [--samplings 420,422,444,gray]
The frames are those of scripts/jpeg_decode_time.py (synth.synth_video at quality 90; gray: the green channel), 854 x 480 and
1920 x 1080, written by Pillow with its defaults (no restart markers: one segment per frame) and with restart_marker_blocks=16.

  stages      device events around ops.jpeg_decode_coefficients (sequential) and ops.jpeg_decode_coefficients_parallel, the bytes
              already on the device, alternating, `repeats` times each after a warm-up; coefficients and status torch.equal
  sweep       the parallel stage at subseq_bytes 32 ... 512 on the two folders without restart markers
  crossover   854 x 480 at 4:2:0 with restart intervals of 1 ... 1024 MCUs: both stages against the mean segment length
  load_video  wall clock, synchronised, warm file cache: DTK_JPEG_DECODE=host against DTK_JPEG_DECODE=device with
              DTK_JPEG_ENTROPY=sequential and =parallel, alternating; the three results torch.equal"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dino_tracker_amd import ops, synth, video_in, video_io  # noqa: E402

DEV = "cuda:0"
SHAPES = {"854x480": (480, 854), "1920x1080": (1080, 1920)}
RESIZE = (476, 854)
SWEEP = (32, 64, 128, 256, 512)
INTERVALS = (1, 4, 16, 64, 256, 1024)
PILLOW = {"420": {}, "422": {"subsampling": 1}, "444": {"subsampling": 0}, "gray": {}}


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


def load(folder, mode, entropy="sequential"):
    os.environ["DTK_JPEG_DECODE"], os.environ["DTK_JPEG_ENTROPY"] = mode, entropy
    try:
        return video_io.load_video(folder, resize=RESIZE, device=DEV)
    finally:
        del os.environ["DTK_JPEG_DECODE"], os.environ["DTK_JPEG_ENTROPY"]


def write_folder(path, frames, sampling, **kw):
    from PIL import Image
    os.makedirs(path)
    for t, f in enumerate(frames):
        Image.fromarray(f[..., 1] if sampling == "gray" else f).save(os.path.join(path, f"{t:05d}.jpg"), quality=90, **PILLOW[sampling], **kw)
    return path


class Folder:
    def __init__(self, folder):
        files = video_io.video_files(folder)
        pinned, views = video_in.read_pinned(files)
        self.plan, why = video_in.plan_jpeg_sampled(views)
        assert self.plan is not None, why
        self.stream = pinned.to(DEV)
        self.huff = torch.from_numpy(self.plan.huffman).to(DEV)

    def sequential(self):
        p = self.plan
        return ops.jpeg_decode_coefficients(self.stream, p.segments, self.huff, p.height, p.width, p.sampling)

    def parallel(self, L=0):
        p = self.plan
        return ops.jpeg_decode_coefficients_parallel(self.stream, p.segments, self.huff, p.height, p.width, p.sampling, L)

    def describe(self):
        p = self.plan
        return {"sampling": video_in.SAMPLING_NAMES[p.sampling], "frames": p.frames, "bytes": int(self.stream.numel()),
                "segments_per_frame": p.segments.shape[0] // p.frames, "mean_segment_bytes": float(p.segments[:, 2].mean())}


def stages(folder, repeats, sweep=False):
    f = Folder(folder)
    want, st = f.sequential()                                                         # warm-up, and the reference
    got, st_p = f.parallel()
    assert not bool(st.any()) and torch.equal(got, want) and torch.equal(st_p, st)
    out = f.describe()
    seq, par = [], []
    for _ in range(repeats):
        seq.append(event_ms(f.sequential))
        par.append(event_ms(f.parallel))
    out.update(sequential_ms=seq, parallel_ms=par, sequential_spread_ms=max(seq) - min(seq),
               parallel_beats_sequential_by_more_than_its_spread=max(par) < min(seq) - (max(seq) - min(seq)))
    if sweep:
        out["sweep_ms"] = {}
        for L in SWEEP:
            got, st_p = f.parallel(L)
            assert torch.equal(got, want) and torch.equal(st_p, st)
            out["sweep_ms"][str(L)] = [event_ms(lambda: f.parallel(L)) for _ in range(repeats)]
    return out


def whole(folder, repeats):
    modes = (("host", "sequential"), ("device", "sequential"), ("device", "parallel"))
    ref = [load(folder, *m) for m in modes]                                            # warm-up
    times = {m: [] for m in modes}
    for _ in range(repeats):
        for m in modes:
            times[m].append(wall_ms(lambda: load(folder, *m)))
    host = times[modes[0]]
    return {"host_ms": host, "device_sequential_ms": times[modes[1]], "device_parallel_ms": times[modes[2]],
            "host_spread_ms": max(host) - min(host), "bit_equal": torch.equal(ref[0], ref[1]) and torch.equal(ref[0], ref[2]),
            "parallel_within_host_spread": float(np.median(times[modes[2]])) <= float(np.median(host)) + max(host) - min(host)}


def main():
    args = sys.argv[1:]
    T = int(args[args.index("--frames") + 1]) if "--frames" in args else 90
    T1080 = int(args[args.index("--frames-1080") + 1]) if "--frames-1080" in args else 30
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 7
    samplings = (args[args.index("--samplings") + 1] if "--samplings" in args else "420,422,444,gray").split(",")
    assert all(s in PILLOW for s in samplings), samplings
    out = {"frames": T, "frames_1080": T1080, "repeats": repeats, "device": torch.cuda.get_device_name(0)}
    for name, (H, W) in SHAPES.items():
        n = T1080 if name == "1920x1080" else T
        frames = synth.synth_video(n, H, W, seed=H).mul(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
        for sampling in samplings:
            with tempfile.TemporaryDirectory() as root:
                plain = write_folder(os.path.join(root, "plain"), frames, sampling)
                rst = write_folder(os.path.join(root, "rst16"), frames, sampling, restart_marker_blocks=16)
                res = {"no_restart": dict(stages(plain, repeats, sweep=True), load_video=whole(plain, repeats)),
                       "restart_16": dict(stages(rst, repeats), load_video=whole(rst, repeats))}
                if sampling == "420" and name == "854x480":
                    res["crossover"] = [stages(write_folder(os.path.join(root, f"r{R}"), frames, sampling, restart_marker_blocks=R), repeats)
                                        for R in INTERVALS]
            out[f"{name}/{sampling}"] = res
            print(json.dumps({f"{name}/{sampling}": res}), flush=True)
            if args and not args[0].startswith("--"):
                with open(args[0], "w") as fh:
                    json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
