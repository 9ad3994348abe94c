"""Step time of the ViT encoder with and without registers (docs/MEASUREMENTS.md, "DINOv2 with registers"), and digests of the plain
model's outputs.

    python scripts/vitreg_time.py [--lib PATH/libdtk.so] [--frames 8] [--layer 11] [--iters 20] [--no-reg]

Encodes `--frames` frames of 854 x 476 through block `--layer` with dinov2_vits14_reg and dinov2_vits14 (seeded weights, LayerScale 0.1 as
the benchmark uses), alternating, and times every pass with device events: median, minimum and maximum of `--iters` passes after three
warm-up passes.  The digests (sha256 of tokens / feat / qkv of three small frames of the PLAIN model, fast and split, both
patch-embedding kernels) are equal between two libraries exactly when those outputs are bit-identical; `--lib` runs the same Python on
another build of the library (`--no-reg` for one that predates the register fields).  Prints one JSON line."""
import argparse
import hashlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dino_tracker_amd import _lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--layer", type=int, default=11)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-reg", action="store_true")
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from dino_tracker_amd.extractor import VitExtractor
    dev = "cuda:0"
    out = {"lib": _lib.LIB_PATH, "frames": a.frames, "layer": a.layer, "iters": a.iters}

    small = synth.synth_video(3, 98, 126, seed=73)
    sd2 = synth.make_vit_weights("dinov2_vits14", seed=9, nblocks=2)
    h = hashlib.sha256()
    for stride in (7, 14):
        for precision in ("fast", "split"):
            ex = VitExtractor("dinov2_vits14", stride=stride, device=dev, state_dict=sd2, precision=precision)
            for layer, want in ((-1, "tokens"), (-1, "feat"), (1, "tokens"), (1, "feat"), (1, "qkv"), (0, "feat")):
                h.update(ex.encode(small, layer=layer, want=want).cpu().numpy().tobytes())
    out["plain_digest"] = h.hexdigest()

    video = synth.synth_video(a.frames, 476, 854, seed=1).to(dev)
    names = ["dinov2_vits14"] + ([] if a.no_reg else ["dinov2_vits14_reg"])
    exs = {n: VitExtractor(n, stride=7, device=dev, state_dict=synth.make_vit_weights(n, seed=2, layerscale=0.1)) for n in names}
    times = {n: [] for n in names}
    for it in range(3 + a.iters):
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            exs[n].encode(video, layer=a.layer, defer_check=True)
            e1.record()
            e1.synchronize()
            exs[n].check_overflow()
            if it >= 3:
                times[n].append(e0.elapsed_time(e1))
    for n in names:
        t = times[n]
        out[n] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                  "tokens_per_frame": 1 + exs[n].n_registers + 67 * 121 if hasattr(exs[n], "n_registers") else 1 + 67 * 121}
    if len(names) == 2:
        out["ratio_reg_over_plain"] = round(out[names[1]]["ms_median"] / out[names[0]]["ms_median"], 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
