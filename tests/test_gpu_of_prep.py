"""MI355X: the optical-flow preprocessing kernels (dtk_traj_start_fg, dtk_nearest_traj, dtk_of_filter_keep) through
dino_tracker_amd.of_preprocessing, against tests/golden/of_prep.npz (the un-modified reference's outputs on seeded inputs) and,
at the headline size, against an ATen restatement on the GPU."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import of_prep_data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "of_prep.npz")
DEV = "cuda:0"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    assert D.digest(D.filter_trajectories()) == str(g["digest_filter_traj"])
    assert D.digest(D.split_trajectories()) == str(g["digest_split_traj"])
    return g


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal on the bit patterns (NaN rows compare equal)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def near_tie(traj_t: torch.Tensor, g: torch.Tensor, a: int, b: int, ulps: int = 2) -> bool:
    """The fp32 distances of candidates a and b from grid point g are within `ulps` ulp."""
    da, db = (torch.linalg.vector_norm(traj_t[n].float().cpu() - g.cpu()) for n in (a, b))
    if not (torch.isfinite(da) and torch.isfinite(db)):
        return False
    hi = torch.maximum(da, db)
    return bool((da - db).abs() <= ulps * (torch.nextafter(hi, torch.tensor(float("inf"))) - hi))


def gold_bb(gold, device=DEV):
    """The best-buddies dict the reference's filter read, rebuilt from the fixture."""
    off = np.concatenate([[0], np.cumsum(gold["bb_sizes"])])
    src, tgt, cos = (torch.from_numpy(gold[k]).to(device) for k in ("bb_source", "bb_target", "bb_cos"))
    peak, r = torch.from_numpy(gold["bb_peak_affs"]).to(device), torch.from_numpy(gold["bb_r"]).to(device)
    bb, q = {}, 0
    for p, (s, t) in enumerate(gold["pairs"].tolist()):
        a, b = int(off[p]), int(off[p + 1])
        e = {"source_coords": src[a:b], "target_coords": tgt[a:b], "cos_sims": cos[a:b]}
        if gold["bb_nms"][p]:
            e.update(peak_coords=None, peak_affs=peak[q:q + b - a], r=r[q:q + b - a])
            q += b - a
        bb[f"{s}_{t}"] = e
    return bb


def test_split_equals_reference(gold):
    from dino_tracker_amd.of_preprocessing import split_trajectories_fg_bg
    from dino_tracker_amd.train import load_masks
    straj = torch.from_numpy(D.split_trajectories())
    with tempfile.TemporaryDirectory() as tmp:
        masks = load_masks(D.write_masks(tmp))
    fg, bg = split_trajectories_fg_bg(straj, masks, DEV)
    isfg = torch.zeros(straj.shape[0], dtype=torch.bool)
    isfg[torch.from_numpy(gold["fg_rows"]).long()] = True
    assert bits_equal(fg.cpu(), straj[isfg]) and bits_equal(bg.cpu(), straj[~isfg])


def test_nearest_equals_reference(gold):
    from dino_tracker_amd.of_preprocessing import nearest_trajectories
    traj = torch.from_numpy(D.filter_trajectories())
    idx = nearest_trajectories(traj, D.H, D.W, D.STRIDE, DEV).cpu()
    want = torch.from_numpy(gold["idx"])
    assert idx.dtype == torch.int64 and idx.shape == want.shape
    grid = torch.from_numpy(D.grid_points())
    diff = (idx != want).nonzero().tolist()
    for t, g in diff:
        assert near_tie(traj[:, t], grid[g], int(idx[t, g]), int(want[t, g])), (t, g, int(idx[t, g]), int(want[t, g]))
    print(f"\nnearest trajectory, golden case: {len(diff)} near ties of {want.numel()} grid points")
    assert len(diff) <= 8


def test_filter_equals_reference(gold):
    from dino_tracker_amd.of_preprocessing import of_filter_best_buddies
    traj = torch.from_numpy(D.filter_trajectories())
    bb = gold_bb(gold)
    out = of_filter_best_buddies(bb, traj, D.H, D.W, D.STRIDE, DEV)
    pairs = gold["pairs"].tolist()
    assert list(out) == [f"{s}_{t}" for s, t in pairs]
    off = np.concatenate([[0], np.cumsum(gold["bb_sizes"])])
    keep = torch.from_numpy(gold["keep"])
    nones = 0
    for p, (s, t) in enumerate(pairs):
        key = f"{s}_{t}"
        k = keep[off[p]:off[p + 1]].to(DEV)
        e, o = bb[key], out[key]
        assert set(o) == {"source_coords", "target_coords", "cos_sims", "peak_coords", "peak_affs", "r"}
        if not bool(k.any()):
            assert all(v is None for v in o.values()), key
            nones += 1
            continue
        for f in ("source_coords", "target_coords", "cos_sims"):
            assert torch.equal(o[f], e[f][k]), (key, f)
        assert o["peak_coords"] is None
        for f in ("peak_affs", "r"):
            if gold["bb_nms"][p]:
                assert torch.equal(o[f], e[f][k]), (key, f)
            else:
                assert o[f] is None, (key, f)
    assert 0 < nones < len(pairs)


def test_edge_cases():
    from dino_tracker_amd.of_preprocessing import nearest_trajectories, split_trajectories_fg_bg
    nan = float("nan")
    # exact ties -> lowest index; a frame with no tracked point -> 0.  Grid of 20 x 20 px: points (7, 7), (14, 7), (7, 14), (14, 14)
    traj = torch.full((6, 3, 2), nan)
    traj[1, 0] = torch.tensor([8.0, 7.0])     # distance 1 from (7, 7)
    traj[4, 0] = torch.tensor([7.0, 8.0])     # distance 1 too: tie -> 1
    traj[2, 0] = torch.tensor([6.0, 7.0])     # distance 1 too, lower index than 4, higher than 1
    traj[5, 0] = torch.tensor([14.0, 14.0])
    traj[3, 0] = torch.tensor([14.0, 14.0])   # exact duplicate: 3 wins over 5
    traj[0, 2] = torch.tensor([100.0, 100.0])
    traj[5, 2] = torch.tensor([100.0, 100.0])
    idx = nearest_trajectories(traj, 20, 20, 7, DEV).cpu()
    assert idx.shape == (3, 4)
    assert idx[0, 0] == 1 and idx[0, 3] == 3
    assert (idx[1] == 0).all()                # frame 1: nothing tracked
    assert (idx[2] == 0).all()                # rows 0 and 5 equidistant everywhere -> 0
    # the split raises on rows without a defined reference result
    masks = torch.zeros((3, 20, 30), dtype=torch.uint8)
    masks[1, 5, 6] = 255
    ok = torch.full((2, 3, 2), nan)
    ok[0, 1] = torch.tensor([6.4, 4.5])       # rint(4.5) = 4 (half to even): background
    ok[1, 1] = torch.tensor([5.5, 5.49])      # rint(5.5) = 6, rint(5.49) = 5: foreground
    fg, bg = split_trajectories_fg_bg(ok, masks, DEV)
    assert bits_equal(fg.cpu(), ok[1:]) and bits_equal(bg.cpu(), ok[:1])
    all_nan = ok.clone()
    all_nan[1] = nan
    with pytest.raises(RuntimeError, match="no tracked frame"):
        split_trajectories_fg_bg(all_nan, masks, DEV)
    outside = ok.clone()
    outside[0, 1] = torch.tensor([29.6, 3.0])  # rounds to x = 30, outside the 30 px mask (the reference would wrap or fault)
    with pytest.raises(RuntimeError, match="outside"):
        split_trajectories_fg_bg(outside, masks, DEV)


def test_nearest_crosses_scan_chunks():
    """66 049 rows are 259 blocks of 256 per frame, so the per-frame offsets scan (nn_scan) carries past its first 256 counts;
    the last tracked row of frame 1 is the only row of the last, partial block.  Tracked rows sit on distinct integer pixels:
    fp32 squared distances are exact, and ties go to the lowest row (test_edge_cases)."""
    from dino_tracker_amd.of_preprocessing import nearest_trajectories
    N, hw, stride = 257 * 257, 32, 7
    traj = np.full((N, 2, 2), np.nan, dtype=np.float32)
    want = []
    grid = D.grid_points(hw, hw, stride)
    for t, (rem, mul) in enumerate(((0, 397), (256, 613))):
        rows = np.nonzero(np.arange(N) % 257 == rem)[0]
        pix = (np.arange(len(rows)) * mul + 5 * t) % (hw * hw)                      # odd multiplier: distinct pixels
        assert len(np.unique(pix)) == len(rows) == 257
        traj[rows, t] = np.stack([pix % hw, pix // hw], axis=1).astype(np.float32)
        d2 = ((traj[rows, t][None] - grid[:, None]) ** 2).sum(-1, dtype=np.float32)
        want.append(rows[d2.argmin(axis=1)])                                        # argmin: the first minimum
    assert bool(np.isfinite(traj[N - 1, 1]).all()) and -(-N // 256) == 259
    idx = nearest_trajectories(torch.from_numpy(traj), hw, hw, stride, DEV).cpu().numpy()
    assert np.array_equal(idx, np.stack(want))


# ---- headline size: T = 90 at 476 x 854, ~1 M trajectories, against ATen on the GPU ---------------------------------------------
def synth_headline(N=1_000_000, T=90, h=476, w=854, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed)
    s0 = torch.randint(0, T - 1, (N,), generator=g, device=DEV)
    length = 2 + (torch.rand(N, generator=g, device=DEV) * (T - s0 - 1).float()).long()
    end = torch.minimum(s0 + length - 1, torch.tensor(T - 1, device=DEV))
    p = torch.stack([torch.randint(0, w, (N,), generator=g, device=DEV), torch.randint(0, h, (N,), generator=g, device=DEV)], 1).float()
    coef = (torch.rand((T, 2, 3), generator=g, device=DEV) - 0.5) * 6
    traj = torch.full((N, T, 2), float("nan"), device=DEV)
    for t in range(T):
        live = (t >= s0) & (t <= end)
        traj[:, t] = torch.where(live[:, None], p, traj[:, t])
        c = coef[t]
        flow = c[:, 0] + c[:, 1] * p[:, :1] / w + c[:, 2] * p[:, 1:] / h
        p = torch.where((t >= s0)[:, None], p + flow, p)
    return traj


def aten_nearest(traj: torch.Tensor, grid: torch.Tensor, rows: int = 256) -> torch.Tensor:
    out = []
    for t in range(traj.shape[1]):
        pts = traj[:, t]
        parts = []
        for i in range(0, grid.shape[0], rows):
            d = torch.linalg.vector_norm(pts[None] - grid[i:i + rows, None], dim=2)
            parts.append(torch.nan_to_num(d, nan=torch.inf).argmin(dim=1))
        out.append(torch.cat(parts))
    return torch.stack(out)


def aten_keep(traj, idx, gw, src, tgt, pair_of, pairs):
    lost = traj.isnan().any(-1)
    s, t = pairs[pair_of, 0], pairs[pair_of, 1]
    cs = torch.div(src - 7, 7, rounding_mode="floor").long()
    ct = torch.div(tgt - 7, 7, rounding_mode="floor").long()
    ns = idx[s, cs[:, 1] * gw + cs[:, 0]]
    nt = idx[t, ct[:, 1] * gw + ct[:, 0]]
    return lost[ns, t] & lost[nt, s]


def test_headline_size_matches_aten():
    from dino_tracker_amd import ops
    from dino_tracker_amd.best_buddies import create_meshgrid
    from dino_tracker_amd.of_preprocessing import ORIGIN, grid_dims, nearest_trajectories
    T, h, w = 90, 476, 854
    traj = synth_headline(T=T, h=h, w=w)
    gh, gw = grid_dims(h, w)
    grid = create_meshgrid(h, w, 7, 14, DEV)
    idx = nearest_trajectories(traj, h, w, 7, DEV)
    want = aten_nearest(traj, grid)
    diff = (idx != want).nonzero()
    for t, g in diff.tolist()[:2000]:
        assert near_tie(traj[:, t], grid[g], int(idx[t, g]), int(want[t, g])), (t, g)
    print(f"\nheadline nearest: {diff.shape[0]} near ties of {want.numel()}")
    assert diff.shape[0] <= 2000
    # synthetic best buddies: 400 random cell pairs per frame pair, every pair in one call
    gen = torch.Generator(device=DEV).manual_seed(9)
    pairs = torch.tensor([(s, t) for s in range(T) for t in range(T) if s != t], dtype=torch.int32, device=DEV)
    per = 400
    P = pairs.shape[0]
    src = grid[torch.randint(0, gh * gw, (P * per,), generator=gen, device=DEV)]
    tgt = grid[torch.randint(0, gh * gw, (P * per,), generator=gen, device=DEV)]
    pair_off = torch.arange(0, P * per + 1, per, dtype=torch.int32, device=DEV)
    keep, err = ops.of_filter_keep(traj, idx.int(), gh, gw, ORIGIN, 7, src, tgt, pair_off, pairs)
    assert int(err.item()) == 0
    pair_of = torch.arange(P, device=DEV).repeat_interleave(per)
    assert torch.equal(keep, aten_keep(traj, idx, gw, src, tgt, pair_of, pairs.long()))
    k_ref = aten_keep(traj, want, gw, src, tgt, pair_of, pairs.long())
    moved = (keep != k_ref).nonzero().flatten()
    if moved.numel():   # only where a buddy's cell is one of the near-tie cells
        tie_cells = set(map(tuple, diff.tolist()))
        for e in moved.tolist()[:200]:
            s, t = pairs[pair_of[e]].tolist()
            cs = torch.div(src[e] - 7, 7, rounding_mode="floor").long().tolist()
            ct = torch.div(tgt[e] - 7, 7, rounding_mode="floor").long().tolist()
            assert (s, cs[1] * gw + cs[0]) in tie_cells or (t, ct[1] * gw + ct[0]) in tie_cells
    print(f"headline filter: {int(keep.sum())} of {keep.numel()} kept, {moved.numel()} moved by near ties")


def test_cli_all_round_trip():
    from dino_tracker_amd import synth
    from dino_tracker_amd.best_buddies import compute_bb_nms_all, extract_best_buddies
    from dino_tracker_amd.of_preprocessing import of_filter_best_buddies, split_trajectories_fg_bg
    from dino_tracker_amd.train import load_masks
    with tempfile.TemporaryDirectory() as data:
        j = os.path.join
        os.makedirs(j(data, "of_trajectories"))
        os.makedirs(j(data, "dino_embeddings"))
        straj = torch.from_numpy(D.split_trajectories())
        torch.save(straj, j(data, "of_trajectories", "trajectories.pt"))
        unf = straj.clone()
        unf[::3, 2] = float("nan")
        torch.save(unf, j(data, "of_trajectories", "trajectories_wo_direct_filter.pt"))
        D.write_masks(j(data, "masks"))
        feats = synth.synth_features(D.T, 32, 67, 121, seed=3)
        torch.save(feats, j(data, "dino_embeddings", "dino_embed_video.pt"))
        cfg = j(data, "preprocessing.yaml")
        with open(cfg, "w") as fh:
            fh.write("video_resh: 476\nvideo_resw: 854\ndino_stride: 7\ndino_bb_box_size: 30\ndino_bb_iou_threshold: 0.2\n")
        env = dict(os.environ, PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, "-m", "dino_tracker_amd.of_preprocessing", "all", "--config", cfg, "--data-path", data],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        files = [j(data, "of_trajectories", "fg_trajectories.pt"), j(data, "of_trajectories", "bg_trajectories.pt"),
                 j(data, "dino_best_buddies", "dino_best_buddies.pt"), j(data, "dino_best_buddies", "dino_best_buddies_filtered.pt")]
        fg_f, bg_f, bb_f, filt_f = (torch.load(f, map_location=DEV) for f in files)
        fg, bg = split_trajectories_fg_bg(straj, load_masks(j(data, "masks")), DEV)
        assert bits_equal(fg_f, fg) and bits_equal(bg_f, bg)
        bb = extract_best_buddies(feats, 476, 854, 7, device=DEV)
        assert list(bb_f) == list(bb)
        for k in bb:
            for f in ("source_coords", "target_coords", "cos_sims"):
                assert torch.equal(bb_f[k][f], bb[k][f]), (k, f)
        filt = compute_bb_nms_all(of_filter_best_buddies(bb, unf, 476, 854, 7, DEV), feats, 476, 854, 7, 30, 0.2, device=DEV)
        assert list(filt_f) == list(filt)
        for k in filt:
            assert set(filt_f[k]) == set(filt[k])
            for f, v in filt[k].items():
                assert (v is None) == (filt_f[k][f] is None), (k, f)
                if v is not None:
                    assert torch.equal(filt_f[k][f], v), (k, f)
