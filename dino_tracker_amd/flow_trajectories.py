"""Long-range trajectories chained from optical flow on the device: preprocessing/extract_trajectories.py behind its RAFT calls.

* `consistency_masks` -- get_flows_with_masks :75-93: the cycle-consistency error of every consecutive frame pair under a
  threshold, and the forward-warp scatter ("some pixel of the previous frame lands here"), on `dtk_flow_cycle_masks`.
* `chain_trajectories` -- save_trajectories :203-266: for every starting frame the start mask with the look-behind rule, the walk of
  every live pixel through all later frames, the optional direct-flow filter (compute_direct_flows_for_start_frame :143-158) and
  the minimum-length compaction, on `dtk_flow_traj_start` / `dtk_flow_traj_emit`.  One host read per starting frame (the row
  count that sizes the block); the blocks are concatenated in start order, which is the reference's row order.
* `extract_trajectories` -- the whole script for a video and a flow network `flow_fn(src, dst) -> flow`, batched as the
  reference batches RAFT.  `raft.raft_flow_fn` makes such a function from this library's RAFT-large (dtk_raft_forward) and a
  weights file; `torchvision_raft` makes one from torchvision's raft_large.

The arithmetic of the device entries is written out in include/dtk.h; tests/traj_ref.py restates it with one ATen operation per
step and the GPU tests ask for the same bits.

Command line (the reference script's flags, plus --flows-path):
    python -m dino_tracker_amd.flow_trajectories --frames-path F --output-path O [--infer-res-size H W] [--threshold 1]
        [--min-trajectory-length 2] [--filter-using-direct-flow --direct-flow-threshold X] [--flows-path P] [--raft-weights W]
--flows-path reads a torch.save'd dict {"forward": [T - 1, 2, h, w], "backward": [T - 1, 2, h, w][, "direct": a list with, per
starting frame, (forward, backward) flows [T - 1 - s, 2, h, w] to every later frame]} instead of running a flow network, so
torchvision is not needed; --frames-path may then be omitted.
--raft-weights W (or the environment variable DTK_RAFT_WEIGHTS) runs the device RAFT-large (dino_tracker_amd.raft) on a state dict
with torchvision's raft_large key names; without either the flows come from torchvision_raft as before.
"""
from __future__ import annotations

import argparse
import os
from typing import Callable, Optional, Tuple

import torch

from . import ops

DirectFlows = Callable[[int], Tuple[torch.Tensor, torch.Tensor]]
FlowFn = Callable[[torch.Tensor, torch.Tensor], torch.Tensor]
DIRECT_BATCH = 16   # compute_direct_flows_for_start_frame's max_batch_size


def _flows_on(flow: torch.Tensor, device) -> torch.Tensor:
    flow = torch.as_tensor(flow)
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError(f"flows must be [n, 2, h, w], got {tuple(flow.shape)}")
    return flow.to(device=device, dtype=torch.float32).contiguous()


def _packed_pair(fflow, bflow, device) -> Tuple[torch.Tensor, torch.Tensor]:
    f, b = _flows_on(fflow, device), _flows_on(bflow, device)
    if f.shape != b.shape:
        raise ValueError(f"forward and backward flows differ in shape: {tuple(f.shape)} and {tuple(b.shape)}")
    if f.shape[0] < 1 or f.shape[2] < 2 or f.shape[3] < 2:
        raise ValueError(f"need at least two frames of at least 2 x 2 pixels, got flows {tuple(f.shape)}")
    return ops.flow_pack(f), ops.flow_pack(b)


@torch.no_grad()
def consistency_masks(fflow: torch.Tensor, bflow: torch.Tensor, threshold: float = 1.0, device="cuda:0") -> torch.Tensor:
    """fflow / bflow [T - 1, 2, h, w] (frame i -> i + 1 and i + 1 -> i) -> consistent [T, h, w] bool on the device: the reference's
    masks_array (cycle error < threshold and hit by the forward warp; frame 0 all False)."""
    fpk, bpk = _packed_pair(fflow, bflow, device)
    return ops.flow_cycle_masks(fpk, bpk, threshold).bool()


@torch.no_grad()
def chain_trajectories(fflow: torch.Tensor, bflow: torch.Tensor, threshold: float = 1.0, min_trajectory_length: int = 2,
                       direct_flows: Optional[DirectFlows] = None, direct_flow_threshold: Optional[float] = None,
                       device="cuda:0") -> torch.Tensor:
    """Trajectories [N, T, 2] fp32 on the device (NaN where a point is not tracked), in the reference's row order.

    direct_flows: a callable s -> (forward, backward), the flows from frame s to each later frame and back, [T - 1 - s, 2, h, w]
    each; it is called once per starting frame (all of them at once do not fit: ~20 GB at 90 frames of 476 x 854) and must come
    together with direct_flow_threshold."""
    if (direct_flows is None) != (direct_flow_threshold is None):
        raise ValueError("direct_flows and direct_flow_threshold come together")
    fpk, bpk = _packed_pair(fflow, bflow, device)
    T, h, w = fpk.shape[0] + 1, fpk.shape[1], fpk.shape[2]
    if not 1 <= min_trajectory_length <= T:
        raise ValueError(f"min_trajectory_length {min_trajectory_length} outside [1, {T}]")
    consistent = ops.flow_cycle_masks(fpk, bpk, threshold)
    visited = torch.zeros((T, h, w), dtype=torch.uint8, device=device)
    ws = ops.flow_traj_workspace(T, h, w, device)
    n_rows = torch.zeros(1, dtype=torch.int32, device=device)
    blocks = []
    for s in range(T - (min_trajectory_length - 1)):
        direct = None
        if direct_flows is not None and s < T - 1:
            df, db = direct_flows(s)
            direct = (ops.flow_pack(_flows_on(df, device)), ops.flow_pack(_flows_on(db, device)))
        ops.flow_traj_start(fpk, bpk, consistent, visited, s, threshold, min_trajectory_length, ws, n_rows, direct,
                            direct_flow_threshold)
        n = int(n_rows.item())   # the one host read of this starting frame
        if n:
            blocks.append(ops.flow_traj_emit(T, h, w, s, min_trajectory_length, n, visited, ws))
    if not blocks:
        return torch.empty((0, T, 2), dtype=torch.float32, device=device)
    return torch.cat(blocks) if len(blocks) > 1 else blocks[0]


def _batched(flow_fn: FlowFn, src: torch.Tensor, dst: torch.Tensor, batch: int) -> torch.Tensor:
    return torch.cat([flow_fn(src[i:i + batch], dst[i:i + batch]) for i in range(0, src.shape[0], batch)])


@torch.no_grad()
def extract_trajectories(video: torch.Tensor, flow_fn: FlowFn, threshold: float = 1.0, min_trajectory_length: int = 2,
                         filter_using_direct_flow: bool = False, direct_flow_threshold: Optional[float] = None,
                         device="cuda:0") -> torch.Tensor:
    """video [T, 3, h, w] in [0, 1]; flow_fn(src [B, 3, h, w], dst [B, 3, h, w]) -> [B, 2, h, w], the flow from src to dst at the
    video's resolution.  Batches as the reference does: each consecutive pair both ways in one call of two, the direct flows
    of a starting frame in chunks of 16."""
    if filter_using_direct_flow and direct_flow_threshold is None:
        raise ValueError("--filter-using-direct-flow needs --direct-flow-threshold")
    video = video.to(device=device, dtype=torch.float32)
    T = video.shape[0]
    if T < 2:
        raise ValueError("need at least two frames")
    pairs = []
    for i in range(T - 1):
        both = torch.stack((video[i], video[i + 1]))
        pairs.append(flow_fn(both, both.flip(0)))
    fflow = torch.stack([p[0] for p in pairs])
    bflow = torch.stack([p[1] for p in pairs])

    def direct(s: int):
        dst = video[s + 1:]
        src = video[s:s + 1].expand_as(dst)
        return _batched(flow_fn, src, dst, DIRECT_BATCH), _batched(flow_fn, dst, src, DIRECT_BATCH)

    return chain_trajectories(fflow, bflow, threshold, min_trajectory_length, direct if filter_using_direct_flow else None,
                              direct_flow_threshold if filter_using_direct_flow else None, device)


def torchvision_raft(device="cuda:0", num_flow_updates: int = 24) -> FlowFn:
    """A flow_fn from torchvision.models.optical_flow.raft_large (default weights, 24 updates), with the reference's padding:
    frames are replicate-padded to multiples of 8 (data_utils.InputPadder, "sintel" mode), mapped to [-1, 1] by the weights'
    transforms, and the flow is cropped back.  torchvision is imported here, lazily; it is not part of this project's test
    environment, so this adapter is NOT covered by the test suite."""
    from torchvision.models.optical_flow import Raft_Large_Weights, raft_large
    model = raft_large(weights=Raft_Large_Weights.DEFAULT, progress=False).to(device).eval()
    transforms = Raft_Large_Weights.DEFAULT.transforms()

    @torch.no_grad()
    def flow_fn(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
        h, w = src.shape[-2:]
        ph, pw = (((h // 8) + 1) * 8 - h) % 8, (((w // 8) + 1) * 8 - w) % 8
        pad = [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2]
        a, b = (torch.nn.functional.pad(x.to(device), pad, mode="replicate") for x in (src, dst))
        a, b = transforms(a, b)
        flow = model(a, b, num_flow_updates=num_flow_updates)[-1]
        return flow[..., pad[2]:flow.shape[-2] - pad[3], pad[0]:flow.shape[-1] - pad[1]].contiguous()

    return flow_fn


def run(frames_path: Optional[str], output_path: str, infer_res_size=None, threshold: float = 1.0, min_trajectory_length: int = 2,
        filter_using_direct_flow: bool = False, direct_flow_threshold: Optional[float] = None, flows_path: Optional[str] = None,
        device="cuda:0", raft_weights=None) -> torch.Tensor:
    """save_trajectories: writes the CPU [N, T, 2] tensor to output_path and prints the reference's line.  raft_weights (a state
    dict or a path; default: the environment variable DTK_RAFT_WEIGHTS) selects the device RAFT-large for the flows."""
    if filter_using_direct_flow and direct_flow_threshold is None:
        raise ValueError("--filter-using-direct-flow needs --direct-flow-threshold")
    if flows_path is not None:
        flows = torch.load(flows_path, map_location="cpu")
        direct = None
        if filter_using_direct_flow:
            if "direct" not in flows:
                raise KeyError(f"{flows_path} has no 'direct' flows, which --filter-using-direct-flow needs")
            direct = lambda s: flows["direct"][s]   # noqa: E731
        traj = chain_trajectories(flows["forward"], flows["backward"], threshold, min_trajectory_length, direct,
                                  direct_flow_threshold if filter_using_direct_flow else None, device)
    else:
        if frames_path is None:
            raise ValueError("--frames-path or --flows-path is required")
        from .train import load_video
        video = load_video(frames_path, resize=tuple(infer_res_size) if infer_res_size is not None else None, device=device)
        if raft_weights is None:
            raft_weights = os.environ.get("DTK_RAFT_WEIGHTS") or None
        if raft_weights is not None:
            from .raft import RaftLarge, raft_flow_fn
            flow_fn = raft_flow_fn(RaftLarge(raft_weights, device))
        else:
            flow_fn = torchvision_raft(device)
        traj = extract_trajectories(video, flow_fn, threshold, min_trajectory_length, filter_using_direct_flow,
                                    direct_flow_threshold, device)
    traj = traj.cpu()
    d = os.path.dirname(output_path)
    if d:
        os.makedirs(d, exist_ok=True)
    torch.save(traj, output_path)
    print(f"Saved {output_path}, shape: {traj.shape}")
    return traj


def main(argv=None):
    ap = argparse.ArgumentParser(prog="dino_tracker_amd.flow_trajectories")
    ap.add_argument("--frames-path", type=str, default=None, help="Path to frames folder")
    ap.add_argument("--output-path", type=str, required=True)
    ap.add_argument("--infer-res-size", type=int, nargs=2, default=None, help="Inference resolution size, (h, w)")
    ap.add_argument("--threshold", type=float, default=1, help="Threshold for cycle consistency error")
    ap.add_argument("--min-trajectory-length", type=int, default=2, help="Minimum trajectory length")
    ap.add_argument("--filter-using-direct-flow", action="store_true", default=False, help="Filter using direct flow")
    ap.add_argument("--direct-flow-threshold", type=float, default=None, help="Threshold for direct flow error")
    ap.add_argument("--flows-path", type=str, default=None, help="torch.save'd flows to chain instead of running RAFT")
    ap.add_argument("--raft-weights", type=str, default=None,
                    help="raft_large state dict for the device RAFT (default: $DTK_RAFT_WEIGHTS, else torchvision)")
    a = ap.parse_args(argv)
    run(a.frames_path, a.output_path, a.infer_res_size, a.threshold, a.min_trajectory_length, a.filter_using_direct_flow,
        a.direct_flow_threshold, a.flows_path, raft_weights=a.raft_weights)


if __name__ == "__main__":
    main()
