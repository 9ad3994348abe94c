"""Timings of the PCA foreground-mask launches (docs/MEASUREMENTS.md): T = 90 frames of 67 x 121 tokens (N = 729 630), C = 1024 and
384, beside their floors and beside the reference's torch.pca_lowrank path on the same device tensor.
    python scripts/fg_mask_time.py [out.json]
Call times: device events around each call, after a warm-up.  Kernel times: the library's own per-launch events, a pass of its own."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dino_tracker_amd import fg_mask, ops  # noqa: E402

DEV = "cuda:0"
T, h, w, H, W = 90, 67, 121, 476, 854
N = T * h * w
out = {"N": N}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


for C in (1024, 384):
    g = torch.Generator(device=DEV).manual_seed(C)
    x = torch.randn(N, C, generator=g, device=DEV) * 0.5 + torch.randn(C, generator=g, device=DEV)[None] * 1.5
    x[: N // 5] += torch.randn(C, generator=g, device=DEV)[None]
    r = {}
    r["moments_ms"] = timed(lambda: ops.pca_moments(x), 6)
    mean, cov = ops.pca_moments(x)
    V, ev = fg_mask.principal_components(cov, 3)
    Vd = V.float().to(DEV).contiguous()
    r["project_ms"] = timed(lambda: ops.pca_project(x, Vd), 6)
    colors, minmax = ops.pca_project(x, Vd)
    r["fg_mask_ms"] = timed(lambda: ops.fg_mask(colors, minmax, (T, h, w), (H, W), 0.6), 6)
    # per-kernel split (hipEvents around every launch inside the library), a run of its own
    ops.profile_enable(True)
    for _ in range(4):
        ops.pca_moments(x)
        ops.pca_project(x, Vd)
        ops.fg_mask(colors, minmax, (T, h, w), (H, W), 0.6)
    prof = ops.profile_collect()
    ops.profile_enable(False)
    r["kernels_ms_per_launch"] = {k: v[0] / max(v[1], 1) for k, v in prof.items() if k.startswith(("pca_", "fg_"))}
    t0 = time.perf_counter()
    fm = x.view(T, h, w, C)
    fg_mask.get_fg_mask_from_pca(fm, (H, W), fg_mask_threshold=0.6)
    torch.cuda.synchronize()
    r["end_to_end_s_with_host_eigh_and_d2h"] = time.perf_counter() - t0
    # floors
    flop = 3 * 2 * N * C * C / 2
    r["moments_floor_ms"] = {"mfma_fp16_2.5PF": flop / 2.5e15 * 1e3, "hbm_two_reads_6.3TBs": 2 * N * C * 4 / 6.3e12 * 1e3}
    r["project_floor_ms"] = {"hbm_one_read_6.3TBs": N * C * 4 / 6.3e12 * 1e3}

    # the reference's path on the same device tensor
    def ref():
        f = torch.nn.functional.normalize(x, dim=-1)
        m = torch.pca_lowrank(f, q=3, niter=20)[2]
        c = f @ m
        return (c - c.min(dim=0).values) / (c.max(dim=0).values - c.min(dim=0).values)
    torch.manual_seed(0)
    r["reference_pca_lowrank_ms"] = timed(ref, 2)
    c_ref = ref()[:, 0]
    c_dev = ((colors[:, 0] - minmax[0]) / (minmax[8] - minmax[0]))
    r["max_abs_color_diff_vs_reference"] = float(min((c_ref - c_dev).abs().max(), (c_ref - (1 - c_dev)).abs().max()))
    r["lambda2_over_lambda1"] = float(ev[1] / ev[0])
    out[f"C{C}"] = r
    print(C, json.dumps(r), flush=True)
    del x, colors, fm

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
