"""Times the flow-trajectory chaining (dino_tracker_amd.flow_trajectories) on one GPU at T = 90 frames of 476 x 854, on flows built
like tests/golden/traj_data.smooth (an affine motion per frame, 0.15 px noise, a disc of 12 x the noise; direct flows = composed
maps + noise + a drift on one side): consistency masks + chaining without and with the direct-flow filter.  The flows are generated
on the device with torch, not with traj_data.smooth on the host: the direct flows of all starting frames are 2 x 4 005 fields of
3.25 MB (26 GB), and numpy would draw 6.5 G random numbers and copy them over for one timed run; the construction is the same, the
random numbers are not (nothing here compares values with the tests' cases).

    python scripts/flow_traj_time.py [--frames 90] [--skip-aten] [--no-events] [--out FILE.json]

Device seconds are the library's per-launch events (dtk_profile_*) summed over the flow_* kernels; the call time is a host clock
around a device synchronise and, with the filter, includes generating the direct flows (timed on their own as well).  The ATen
column runs tests/traj_ref.py -- the same arithmetic, one ATen operation per step, the stand-in for the reference's loop -- for
ONE starting frame on the same GPU and scales it by the step count (sum over s of T - 1 - s against T - 1).  With --no-events
and --skip-aten the script is a plain workload for `rocprofv3 --kernel-trace --stats -- python scripts/flow_traj_time.py ...`.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dino_tracker_amd import flow_trajectories as FT, ops  # noqa: E402

DEV = "cuda:0"
H, W = 476, 854
THRESHOLD, DIRECT_THRESHOLD = 1.0, 1.5


class Smooth:
    """traj_data.smooth's construction with torch on the device (float64 arithmetic, one rounding to float32)"""

    def __init__(self, T, seed=90):
        self.T = T
        self.g = torch.Generator(device=DEV).manual_seed(seed)
        yy, xx = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float64), torch.arange(W, device=DEV, dtype=torch.float64),
                                indexing="ij")
        self.xx, self.yy = xx, yy
        self.disc = (xx - 0.3 * W) ** 2 + (yy - 0.55 * H) ** 2 < (0.16 * min(H, W)) ** 2
        self.right = (xx > 0.6 * W).double()
        cpu = torch.Generator().manual_seed(seed)
        self.maps = []
        for _ in range(T - 1):
            e = (torch.rand(4, generator=cpu, dtype=torch.float64) - 0.5) * 0.06
            a, b, c, d = 1 + e[0].item(), e[1].item(), e[2].item(), 1 + e[3].item()
            t = torch.rand(2, generator=cpu, dtype=torch.float64) - 0.5
            cx, cy = (W - 1) / 2, (H - 1) / 2
            self.maps.append((a, b, cx - (a * cx + b * cy) + 6 * t[0].item(), c, d, cy - (c * cx + d * cy) + 4 * t[1].item()))
        self.fflow = torch.stack([self.field(m) for m in self.maps])
        self.bflow = torch.stack([self.field(self.invert(m)) for m in self.maps])

    def noise(self):
        n = (torch.rand((2, H, W), generator=self.g, device=DEV, dtype=torch.float64) - 0.5) * 0.3
        return torch.where(self.disc, 12.0 * n, n)

    def field(self, p, drift=None):
        a, b, tx, c, d, ty = p
        f = torch.stack([a * self.xx + b * self.yy + tx - self.xx, c * self.xx + d * self.yy + ty - self.yy]) + self.noise()
        return (f if drift is None else f + drift).float()

    @staticmethod
    def invert(p):
        a, b, tx, c, d, ty = p
        det = a * d - b * c
        ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
        return (ia, ib, -(ia * tx + ib * ty), ic, id_, -(ic * tx + id_ * ty))

    @staticmethod
    def compose(q, p):
        a, b, tx, c, d, ty = p
        A, B, TX, C, D, TY = q
        return (A * a + B * c, A * b + B * d, A * tx + B * ty + TX, C * a + D * c, C * b + D * d, C * tx + D * ty + TY)

    def direct(self, s):
        fwd, back, acc = [], [], None
        for k in range(self.T - 1 - s):
            acc = self.maps[s + k] if acc is None else self.compose(self.maps[s + k], acc)
            drift = torch.stack([0.45 * (k + 1) * self.right, -0.2 * (k + 1) * self.right])
            fwd.append(self.field(acc, drift))
            back.append(self.field(self.invert(acc), -drift))
        return torch.stack(fwd), torch.stack(back)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def device_run(case, direct, events):
    """one full consistency-masks + chaining run: call seconds, device seconds per flow_* kernel, rows"""
    extra = (case.direct, DIRECT_THRESHOLD) if direct else (None, None)
    if events:
        ops.profile_enable(True)
    t_call, traj = clock(lambda: FT.chain_trajectories(case.fflow, case.bflow, THRESHOLD, 2, *extra, device=DEV))
    kernels = {}
    if events:
        kernels = {k: v for k, v in ops.profile_collect().items() if k.startswith("flow_")}
        ops.profile_enable(False)
    ok = ~traj.isnan().any(-1)
    return {"call_s": t_call, "device_s": sum(ms for ms, _ in kernels.values()) / 1e3,
            "kernels_ms": {k: [round(ms, 3), n] for k, (ms, n) in sorted(kernels.items())},
            "rows": int(traj.shape[0]), "tracked_points": int(ok.sum()), "mean_length": float(ok.sum(1).float().mean())}


def one_start_device(case, direct, fixed):
    """start frame 0 alone on the library (start + emit): seconds, its rows"""
    T = case.T
    fpk, bpk = ops.flow_pack(case.fflow), ops.flow_pack(case.bflow)
    consistent = ops.flow_cycle_masks(fpk, bpk, THRESHOLD)
    ws = ops.flow_traj_workspace(T, H, W, DEV)
    n_rows = torch.zeros(1, dtype=torch.int32, device=DEV)
    d = tuple(ops.flow_pack(x) for x in fixed) if direct else None

    def run():
        visited = torch.zeros((T, H, W), dtype=torch.uint8, device=DEV)
        ops.flow_traj_start(fpk, bpk, consistent, visited, 0, THRESHOLD, 2, ws, n_rows, d, DIRECT_THRESHOLD if direct else None)
        return ops.flow_traj_emit(T, H, W, 0, 2, int(n_rows.item()), visited, ws)

    rows = run()
    return min(clock(run)[0] for _ in range(3)), rows


def one_start_aten(case, direct, fixed):
    """start frame 0 alone as the restatement's ATen operations on the GPU (its consistency masks timed apart and taken off):
    seconds, the masks' seconds, its rows"""
    import traj_ref as R
    extra = ((lambda s: fixed), DIRECT_THRESHOLD) if direct else (None, None)
    t_masks = min(clock(lambda: R.consistency_masks(case.fflow, case.bflow, THRESHOLD))[0] for _ in range(2))
    runs = [clock(lambda: R.chain_trajectories(case.fflow, case.bflow, THRESHOLD, 2, *extra, starts=[0])) for _ in range(2)]
    return min(t for t, _ in runs) - t_masks, t_masks, runs[0][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=90)
    ap.add_argument("--skip-aten", action="store_true")
    ap.add_argument("--no-events", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "flow_traj_time.py measures on a GPU"
    T = a.frames
    case = Smooth(T)
    steps_all, steps_one = T * (T - 1) // 2, T - 1
    device_run(Smooth(4), True, False)   # warm-up: code objects, allocator
    res = {"device": torch.cuda.get_device_name(0), "T": T, "h": H, "w": W, "steps_all_starts": steps_all}
    for direct in (False, True):
        name = "direct" if direct else "plain"
        row = device_run(case, direct, not a.no_events)
        fixed = case.direct(0) if direct else None   # one draw of start 0's direct flows for both one-start runs
        if direct:
            row["direct_flow_generation_s"] = clock(lambda: [case.direct(s) and None for s in range(T - 1)])[0]
        row["start0_device_s"], rows = one_start_device(case, direct, fixed)
        if not a.skip_aten:
            t_aten, t_masks, want = one_start_aten(case, direct, fixed)
            # the two evaluate the same fp32 operations: equal bits at the headline size, where no CPU test reaches
            row["start0_rows"] = int(rows.shape[0])
            row["start0_bits_equal_aten"] = bool(rows.shape == want.shape and torch.equal(rows.view(torch.int32), want.view(torch.int32)))
            row.update(start0_aten_s=t_aten, aten_masks_s=t_masks, start0_ratio=t_aten / row["start0_device_s"],
                       aten_all_starts_scaled_s=t_aten * steps_all / steps_one)
        res[name] = row
        print(json.dumps({name: row}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
