"""Times the device RAFT-large (dtk_raft_forward through dino_tracker_amd.raft.RaftLarge) on one GPU at 480 x 856 -- the padded
476 x 854 of the preprocessing -- with 24 updates, for batches of 2 and 16 pairs in both operand modes, on seeded weights
(synth.make_raft_weights) and a seeded translating video.

    python scripts/raft_time.py [--batches 2 16] [--updates 24] [--repeats 3] [--out FILE.json]

Per (batch, mode): one warm-up call, then `repeats` calls between two device events (pairs/s from their mean); then ONE more call
with the library's per-launch events on (dtk_profile_*), which gives the per-kernel split.  The events serialise nothing on a
single stream but cost host time per launch, so the split is taken apart from the timed calls.

Derived, from shapes (the code is here): the convolutions' FLOPs (2 x pixels x taps x Cin x Cout, un-padded) over the summed
raft_conv_* kernel time, as a fraction of the split-operand MFMA peak -- the fp16 dense peak / 3, since the split mode issues
three MFMAs per product -- and of the fp16 peak in fp16 mode; and the projected flow time of a 90-frame video: 89 consecutive
pairs both ways, plus with the direct-flow filter the 4 005 (start, later frame) pairs both ways, at the batch-16 rate (the
consecutive pairs at the batch-2 rate, as extract_trajectories batches them).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dino_tracker_amd import ops, synth  # noqa: E402
from dino_tracker_amd.raft import RaftLarge, raft_large_convs  # noqa: E402

DEV = "cuda:0"
H, W = 480, 856
FP16_PEAK = 2.5e15       # dense fp16 MFMA, FLOP/s (MI355X)


def conv_flops(n_pairs: int, updates: int) -> float:
    """FLOPs of every convolution of one dtk_raft_forward call, from the shapes"""
    total = 0.0
    for s in raft_large_convs():
        per_px = 2.0 * s.kh * s.kw * s.cin * s.cout
        if s.key.startswith(("feature_encoder", "context_encoder")):
            imgs = 2 * n_pairs if s.key.startswith("feature_encoder") else n_pairs
            name = s.key.split(".")[1]
            res = 2 if name in ("convnormrelu", "layer1") else 4 if name == "layer2" else 8      # output resolution divisor
            total += per_px * imgs * (H // res) * (W // res)
        else:
            times = 1 if s.key.startswith("mask_predictor") else updates
            total += per_px * n_pairs * (H // 8) * (W // 8) * times
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 16])
    ap.add_argument("--updates", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "raft_time.py measures on a GPU"
    sd = synth.make_raft_weights(0)
    nmax = max(a.batches)
    video = synth.synth_video(nmax + 1, H, W, seed=3).to(DEV) * 2 - 1
    res = {"device": torch.cuda.get_device_name(0), "H": H, "W": W, "updates": a.updates, "runs": []}
    rate = {}
    for mode in ("split", "fp16"):
        model = RaftLarge(sd, DEV, operands=mode, max_workspace_bytes=64 << 30)
        for n in a.batches:
            src, dst = video[:n].contiguous(), video[1:n + 1].contiguous()
            model.flow(src, dst, a.updates)      # warm-up: code objects, the workspace
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.repeats):
                model.flow(src, dst, a.updates)
            e1.record()
            torch.cuda.synchronize()
            call_s = e0.elapsed_time(e1) / 1e3 / a.repeats
            ops.profile_enable(True)
            model.flow(src, dst, a.updates)
            kernels = {k: v for k, v in ops.profile_collect().items() if k.startswith("raft_")}
            ops.profile_enable(False)
            conv_s = sum(ms for k, (ms, _) in kernels.items() if k.startswith("raft_conv")) / 1e3
            flops = conv_flops(n, a.updates)
            peak = FP16_PEAK / 3 if mode == "split" else FP16_PEAK
            row = {"mode": mode, "pairs": n, "call_s": call_s, "pairs_per_s": n / call_s, "workspace_gb": model.workspace_bytes(n, H, W) / 2 ** 30,
                   "kernels_ms": {k: [round(ms, 3), cnt] for k, (ms, cnt) in sorted(kernels.items())},
                   "kernel_sum_s": sum(ms for ms, _ in kernels.values()) / 1e3, "conv_kernel_s": conv_s, "conv_tflop": flops / 1e12,
                   "conv_tflops": flops / conv_s / 1e12, "conv_fraction_of_mode_peak": flops / conv_s / peak}
            rate[mode, n] = n / call_s
            res["runs"].append(row)
            print(json.dumps(row), flush=True)
        del model
        torch.cuda.empty_cache()
    for mode in ("split", "fp16"):
        if (mode, 2) in rate and (mode, 16) in rate:
            consecutive = 2 * 89 / rate[mode, 2]
            direct = 2 * 4005 / rate[mode, 16]
            proj = {"mode": mode, "video_90_frames_flow_s": consecutive, "video_90_frames_with_direct_filter_s": consecutive + direct}
            res.setdefault("projection", []).append(proj)
            print(json.dumps(proj), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
