"""Optical-flow preprocessing on the device: the fg / bg split of the RAFT trajectories and the optical-flow filter of the DINO
best buddies -- the two steps between the trajectories and the training loop that still needed the reference checkout.

* `split_trajectories_fg_bg` -- preprocessing/split_trajectories_to_fg_bg.py:55-76 (`mask_filter_trajectories` twice): the mask
  at each trajectory's first tracked point (`generate_start_end` + argmax, rounded half-to-even) on `dtk_traj_start_fg`; rows
  keep their input order (boolean indexing, like the reference).
* `nearest_trajectories` -- of_filter_dino_best_buddies.py:9-29, :50-54: for every frame the nearest trajectory of every token-grid
  point, all frames in one `dtk_nearest_traj` call (lowest index on equal fp32 distances, untracked points at +inf).
* `of_filter_best_buddies` -- of_filter_dino_best_buddies.py:61-105: the keep flag of every buddy of every frame pair in one
  `dtk_of_filter_keep` call, compaction by one boolean index per field.  The reference keeps a buddy when BOTH flow
  trajectories are lost at the other frame; restated as written.

Rows the reference has no defined result for (a trajectory with no tracked frame or a start point outside the mask, a buddy
outside the token grid) raise instead of wrapping an index silently.

Command lines (the reference scripts' flags):
    python -m dino_tracker_amd.of_preprocessing split --traj_path T --fg_masks_path M --fg_traj_path F --bg_traj_path B
    python -m dino_tracker_amd.of_preprocessing of-filter --dino-bb-path P --traj-path T --out-path O [--dino-bb-stride 7 --h --w]
    python -m dino_tracker_amd.of_preprocessing masks --config config/preprocessing.yaml --data-path D
    python -m dino_tracker_amd.of_preprocessing all --config config/preprocessing.yaml --data-path D [--make-masks]
`masks` writes the PCA foreground masks (dino_tracker_amd.fg_mask; main_preprocessing.py step 3) from the mask embedding file.
`all` runs split, best-buddy extraction, optical-flow filter and NMS ratios (main_preprocessing.py step 4 and
main_dino_bb_preprocessing.py steps 1, 3, 4) with the tensors on the device between steps, and writes the reference's files.  With --make-masks it first builds the masks
when the mask folder is missing -- from the mask embedding file if present, otherwise from the video; without the flag a missing
mask folder is an error, as before.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, Optional, Tuple

import torch

from . import ops

ORIGIN = 7          # the literal of of_filter_dino_best_buddies.py:83 and create_meshgrid's patch_size // 2
FIELDS = ("source_coords", "target_coords", "cos_sims")
CARRIED = ("peak_coords", "peak_affs", "r")


def grid_dims(h: int, w: int, stride: int = 7, patch_size: int = 14) -> Tuple[int, int]:
    """(rows, columns) of dino_bb_utils.create_meshgrid(h, w, step=stride): arange(patch_size // 2, h | w, stride)."""
    start = patch_size // 2
    return len(range(start, h, stride)), len(range(start, w, stride))


def _traj_on(trajectories: torch.Tensor, device) -> torch.Tensor:
    return trajectories.to(device=device, dtype=torch.float32).contiguous()


@torch.no_grad()
def split_trajectories_fg_bg(trajectories: torch.Tensor, masks, device="cuda:0") -> Tuple[torch.Tensor, torch.Tensor]:
    """trajectories [N, T, 2] (NaN = untracked), masks [T', H, W] (train.load_masks: nearest-resized to 476 x 854) ->
    (fg, bg) rows on the device, in input order: fg where the mask at the trajectory's first tracked point is > 0."""
    masks = torch.as_tensor(masks)
    traj = _traj_on(trajectories, device)
    fg, err = ops.traj_start_fg(traj, masks.to(device=device, dtype=torch.uint8).contiguous())
    nerr = int(err.item())
    if nerr:
        raise RuntimeError(f"split_trajectories_fg_bg: {nerr} trajectories have no tracked frame or start outside the "
                           f"{masks.shape[1]}x{masks.shape[2]} masks (the reference would index with NaN-cast or wrapping indices)")
    return traj[fg], traj[~fg]


@torch.no_grad()
def nearest_trajectories(trajectories: torch.Tensor, h: int, w: int, stride: int = 7, device="cuda:0") -> torch.Tensor:
    """idx [T, G] int64: get_closest_traj_idx_batch for every frame t over the token grid of create_meshgrid(h, w, stride)
    (G = rows x columns, row-major) -- the trajectory nearest to each grid point at t, the lowest index on ties, 0 when frame t
    has no tracked point."""
    gh, gw = grid_dims(h, w, stride)
    return ops.nearest_traj(_traj_on(trajectories, device), gh, gw, ORIGIN, stride).long()


def _pair_keys(T: int):
    return [(s, t) for s in range(T) for t in range(T) if s != t]


@torch.no_grad()
def of_filter_best_buddies(dino_bb: Dict[str, Dict[str, Optional[torch.Tensor]]], trajectories: torch.Tensor, h: int = 476,
                           w: int = 854, stride: int = 7, device="cuda:0",
                           idx: Optional[torch.Tensor] = None) -> Dict[str, Dict[str, Optional[torch.Tensor]]]:
    """of_filter_dino_best_buddies.run on a best-buddies dict: every f"{s}_{t}" key of the T (T - 1) frame pairs gets
    source_coords / target_coords / cos_sims, and peak_coords / peak_affs / r where the input pair has them, restricted to the
    kept buddies -- all six None when a pair keeps nothing.  Values stay on the device they came on."""
    traj = _traj_on(trajectories, device)
    N, T = traj.shape[0], traj.shape[1]
    gh, gw = grid_dims(h, w, stride)
    if idx is None:
        idx32 = ops.nearest_traj(traj, gh, gw, ORIGIN, stride)
    else:
        idx32 = idx.to(device=device, dtype=torch.int32).contiguous()
    pairs = _pair_keys(T)
    entries = []
    for s, t in pairs:
        key = f"{s}_{t}"
        if key not in dino_bb:
            raise KeyError(f"best buddies have no pair {key!r} (the trajectories have {T} frames)")
        entries.append(dino_bb[key])
    sizes = [0 if e.get("source_coords") is None else int(e["source_coords"].shape[0]) for e in entries]
    M = sum(sizes)

    def cat(field):
        parts = [e[field].to(device=device, dtype=torch.float32).reshape(-1, 2) for e, n in zip(entries, sizes) if n]
        return torch.cat(parts).contiguous() if parts else torch.empty((0, 2), dtype=torch.float32, device=device)

    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    pair_off = torch.tensor(offs, dtype=torch.int32, device=device)
    pair_st = torch.tensor(pairs, dtype=torch.int32, device=device).reshape(-1, 2)
    keep, err = ops.of_filter_keep(traj, idx32, gh, gw, ORIGIN, stride, cat("source_coords"), cat("target_coords"), pair_off, pair_st)
    nerr = int(err.item())
    if nerr:
        raise RuntimeError(f"of_filter_best_buddies: {nerr} best buddies lie outside the {gh}x{gw} token grid")
    if M:
        pair_id = torch.repeat_interleave(torch.arange(len(pairs), device=device), torch.tensor(sizes, device=device))
        kept = torch.bincount(pair_id, weights=keep.to(torch.float32), minlength=len(pairs)).long().tolist()
    else:
        kept = [0] * len(pairs)

    out = {f"{s}_{t}": {f: None for f in FIELDS + CARRIED} for s, t in pairs}
    for field in FIELDS + CARRIED:
        # the pairs that carry the field and keep something; one boolean index over their concatenation
        sel = [i for i, e in enumerate(entries) if kept[i] and e.get(field) is not None]
        if not sel:
            continue
        vals = torch.cat([entries[i][field] for i in sel])
        k = torch.cat([keep[offs[i]:offs[i + 1]] for i in sel]).to(vals.device)
        for i, v in zip(sel, torch.split(vals[k], [kept[i] for i in sel])):
            s, t = pairs[i]
            out[f"{s}_{t}"][field] = v
    return out


# ---- command lines ----------------------------------------------------------------------------------------------------------
def _need(path: str, script: str) -> str:
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing: the reference's {script} makes it")
    return path


def _save(obj, path: str) -> None:
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    torch.save(obj, path)


def run_split(traj_path: str, masks_path: str, fg_path: str, bg_path: str, device="cuda:0"):
    from .train import load_masks
    trajectories = torch.load(traj_path, map_location="cpu")
    fg, bg = split_trajectories_fg_bg(trajectories, load_masks(masks_path, device=device), device)
    for traj, path in ((fg, fg_path), (bg, bg_path)):
        traj = traj.cpu()
        torch.save(traj, path)
        print(f"Saved {path}, shape: {traj.shape}")
    return fg, bg


def run_of_filter(dino_bb_path: str, traj_path: str, out_path: str, stride: int = 7, h: int = 476, w: int = 854,
                  device="cuda:0"):
    out = of_filter_best_buddies(torch.load(dino_bb_path), torch.load(traj_path, map_location="cpu"), h, w, stride, device)
    _save(out, out_path)
    print(f"Saved filtered best buddies to {out_path}")
    return out


def _load_config(config_path: str, data_path: str):
    import yaml
    from .utils import add_config_paths
    with open(config_path) as fh:
        return add_config_paths(data_path, yaml.safe_load(fh.read()))


def run_masks(config_path: str, data_path: str, device="cuda:0", from_video: bool = False):
    """main_preprocessing.py step 3 (create_fg_mask.py) on the reference's file layout: mask_dino_embed_video_path -> masks_path;
    with `from_video` a missing embedding file is replaced by the video through the device encoder."""
    from . import fg_mask
    config = _load_config(config_path, data_path)
    h, w, thr = config["video_resh"], config["video_resw"], config["fg_mask_threshold"]
    emb_path = config["mask_dino_embed_video_path"]
    if from_video and not os.path.exists(emb_path):
        from .train import load_video
        video = load_video(_need(config["video_folder"], "video frames"), resize=(h, w), device=device)
        _, details = fg_mask.fg_masks_from_video(video, config["mask_dino_model_name"], config["mask_dino_layer"],
                                                 config["mask_dino_stride"], img_size=(h, w), device=device,
                                                 fg_mask_threshold=thr, return_details=True)
        mask = details["mask"]
        print(f"Saved fg. mask to {fg_mask.save_masks(mask, config['masks_path'])}")
        return mask
    _need(emb_path, "preprocessing/save_dino_embed_video.py")
    return fg_mask.run(emb_path, h, w, config["masks_path"], fg_mask_threshold=thr, device=device)


def _make_trajectories(config, path: str, direct: bool, raft_weights, device) -> None:
    """main_preprocessing.py step 1 (and its unfiltered twin) on the device RAFT: extract_trajectories with the config's settings."""
    from . import flow_trajectories
    flow_trajectories.run(config["video_folder"], path, (config["video_resh"], config["video_resw"]), config["threshold"],
                          config["min_trajectory_length"], direct, config["direct_flow_threshold"] if direct else None,
                          device=device, raft_weights=raft_weights)


def run_all(config_path: str, data_path: str, device="cuda:0", make_masks: bool = False, raft_weights=None):
    """main_preprocessing.py step 4 + main_dino_bb_preprocessing.py steps 1, 3, 4 on the reference's file layout.  With
    raft_weights (or the environment variable DTK_RAFT_WEIGHTS) a missing trajectory file is made here by the device RAFT-large
    (main_preprocessing.py step 1); without it a missing file is an error, as before."""
    import yaml
    from .best_buddies import compute_bb_nms_all, extract_best_buddies
    from .train import load_masks
    from .utils import add_config_paths
    with open(config_path) as fh:
        config = add_config_paths(data_path, yaml.safe_load(fh.read()))
    extract = "preprocessing/extract_trajectories.py (or python -m dino_tracker_amd.flow_trajectories)"
    raft_weights = raft_weights if raft_weights is not None else (os.environ.get("DTK_RAFT_WEIGHTS") or None)
    if raft_weights is not None:
        for key, direct in (("trajectories_file", True), ("unfiltered_trajectories_file", False)):
            if not os.path.exists(config[key]):
                _make_trajectories(config, config[key], direct, raft_weights, device)
    traj_path = _need(config["trajectories_file"], extract + " with --filter-using-direct-flow")
    unfiltered_path = _need(config["unfiltered_trajectories_file"], extract + " without --filter-using-direct-flow")
    if make_masks and not os.path.exists(config["masks_path"]):
        run_masks(config_path, data_path, device, from_video=True)
    masks_path = _need(config["masks_path"], "preprocessing/create_fg_mask.py")
    emb_path = _need(config["dino_embed_video_path"], "preprocessing/save_dino_embed_video.py")
    h, w, stride = config["video_resh"], config["video_resw"], config["dino_stride"]

    # 1. split the direct-flow-filtered trajectories to fg / bg
    fg, bg = split_trajectories_fg_bg(torch.load(traj_path, map_location="cpu"), load_masks(masks_path, device=device), device)
    for traj, path in ((fg, config["fg_trajectories_file"]), (bg, config["bg_trajectories_file"])):
        _save(traj.cpu(), path)
    del fg, bg
    # 2. best buddies of the DINO features
    features = torch.load(emb_path, map_location="cpu")
    bb_dir = config["dino_bb_dir"]
    bb = extract_best_buddies(features, h, w, stride, device=device)
    _save(bb, os.path.join(bb_dir, "dino_best_buddies.pt"))
    # 3. optical-flow filter on the unfiltered trajectories
    bb = of_filter_best_buddies(bb, torch.load(unfiltered_path, map_location="cpu"), h, w, stride, device)
    # 4. NMS ambiguity ratios
    bb = compute_bb_nms_all(bb, features, h, w, stride, config["dino_bb_box_size"], config["dino_bb_iou_threshold"],
                            device=device)
    out_path = os.path.join(bb_dir, "dino_best_buddies_filtered.pt")
    _save(bb, out_path)
    print(f"Saved {config['fg_trajectories_file']}, {config['bg_trajectories_file']}, {out_path}")
    return bb


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in ("split", "of-filter", "masks", "all"):
        raise SystemExit("usage: python -m dino_tracker_amd.of_preprocessing {split|of-filter|masks|all} ...")
    cmd, rest = argv[0], argv[1:]
    ap = argparse.ArgumentParser(prog=f"dino_tracker_amd.of_preprocessing {cmd}")
    if cmd == "split":   # preprocessing/split_trajectories_to_fg_bg.py
        ap.add_argument("--traj_path", default="")
        ap.add_argument("--fg_masks_path", default="")
        ap.add_argument("--fg_traj_path", default="")
        ap.add_argument("--bg_traj_path", default="")
        a = ap.parse_args(rest)
        run_split(a.traj_path, a.fg_masks_path, a.fg_traj_path, a.bg_traj_path)
    elif cmd == "of-filter":   # preprocessing_dino_bb/of_filter_dino_best_buddies.py
        ap.add_argument("--dino-bb-path", type=str, required=True)
        ap.add_argument("--traj-path", type=str, required=True)
        ap.add_argument("--out-path", type=str, required=True)
        ap.add_argument("--dino-bb-stride", type=int, default=7)
        ap.add_argument("--h", type=int, default=476)
        ap.add_argument("--w", type=int, default=854)
        a = ap.parse_args(rest)
        run_of_filter(a.dino_bb_path, a.traj_path, a.out_path, a.dino_bb_stride, a.h, a.w)
    else:   # main_preprocessing.py / main_dino_bb_preprocessing.py
        ap.add_argument("--config", default="./config/preprocessing.yaml", type=str)
        ap.add_argument("--data-path", default="./dataset/libby", type=str)
        if cmd == "masks":   # main_preprocessing.py step 3
            a = ap.parse_args(rest)
            run_masks(a.config, a.data_path)
            return
        ap.add_argument("--make-masks", action="store_true")
        ap.add_argument("--raft-weights", type=str, default=None,
                        help="raft_large state dict: make missing trajectory files with the device RAFT (default: $DTK_RAFT_WEIGHTS)")
        a = ap.parse_args(rest)
        run_all(a.config, a.data_path, make_masks=a.make_masks, raft_weights=a.raft_weights)


if __name__ == "__main__":
    main()
