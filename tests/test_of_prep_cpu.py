"""CPU: a test-local restatement of the optical-flow preprocessing (fg / bg split, nearest trajectory per grid point, optical-flow
filter of the best buddies) equals tests/golden/of_prep.npz, which make_golden_of.py wrote from the un-modified reference
scripts; a second check runs the live reference where a checkout is present."""
import os

import numpy as np
import pytest
import torch

import of_prep_data as D

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "of_prep.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def start_frames(traj: np.ndarray) -> np.ndarray:
    """split_trajectories_to_fg_bg.generate_start_end + argmax: the first frame with both coordinates tracked."""
    ok = ~np.isnan(traj).any(-1)
    assert ok.any(1).all()
    return ok.argmax(1)


def split_rows(traj: np.ndarray, masks: np.ndarray) -> np.ndarray:
    s = start_frames(traj)
    p = traj[np.arange(traj.shape[0]), s]
    x, y = np.rint(p[:, 0]).astype(np.int64), np.rint(p[:, 1]).astype(np.int64)   # torch.round: half to even
    Tm, H, W = masks.shape
    assert ((x >= 0) & (x < W) & (y >= 0) & (y < H)).all()
    return np.nonzero(masks[s, y, x] > 0)[0]


def nearest(traj: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
    """[T, G]: argmin over n of the fp32 distance, NaN = +inf, the first index on ties (torch.argmin)."""
    out = []
    for t in range(traj.shape[1]):
        d = torch.linalg.vector_norm(traj[None, :, t, :] - grid[:, None, :], dim=2)
        out.append(torch.nan_to_num(d, nan=torch.inf).argmin(dim=1))
    return torch.stack(out)


def floordiv(a: torch.Tensor, b: int) -> torch.Tensor:
    return torch.div(a, b, rounding_mode="floor")


def keep_mask(traj: torch.Tensor, idx: torch.Tensor, gw: int, src, tgt, s, t, stride=7) -> torch.Tensor:
    lost = traj.isnan().any(-1)
    cs, ct = floordiv(src - 7, stride).long(), floordiv(tgt - 7, stride).long()
    ns = idx[s][cs[:, 1] * gw + cs[:, 0]]
    nt = idx[t][ct[:, 1] * gw + ct[:, 0]]
    return lost[ns, t] & lost[nt, s]


def near_tie(traj_t: torch.Tensor, g: torch.Tensor, a: int, b: int, ulps: int = 2) -> bool:
    da, db = (torch.linalg.vector_norm(traj_t[n] - g) for n in (a, b))
    if not (torch.isfinite(da) and torch.isfinite(db)):
        return False
    hi = torch.maximum(da, db)
    ulp = torch.nextafter(hi, torch.tensor(float("inf"))) - hi
    return bool((da - db).abs() <= ulps * ulp)


def test_inputs_regenerate_bit_identically(gold):
    assert D.digest(D.filter_trajectories()) == str(gold["digest_filter_traj"])
    assert D.digest(D.split_trajectories()) == str(gold["digest_split_traj"])
    assert D.digest(D.mask_frames()) == str(gold["digest_masks"])
    assert D.digest(D.bb_features().numpy()) == str(gold["digest_features"])


def test_golden_covers_the_edge_cases(gold):
    idx = gold["idx"]
    assert (idx[D.EMPTY_FRAME] == 0).all()                       # frame without a tracked point -> argmin of all-inf
    traj, grid = D.filter_trajectories(), D.grid_points()
    for rows, t, gi in D.tie_rows():                             # exact ties -> the lowest row on the grid point
        n = idx[t, gi]
        assert n <= rows.min() and (traj[n, t] == grid[gi]).all()
        assert ((traj[:n, t] == grid[gi]).all(-1) == 0).all()
    sizes, keep = gold["bb_sizes"], gold["keep"]
    kept = np.add.reduceat(keep.astype(np.int64), np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    assert (kept == 0).any() and (kept > 0).any()                # pairs that keep nothing (None) and pairs that keep some
    assert 0 < len(gold["fg_rows"]) < D.N_SPLIT


def test_split_restatement_matches_reference(gold):
    from dino_tracker_amd.train import load_masks
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        masks = load_masks(D.write_masks(tmp)).numpy()
    assert masks.shape == (D.T, D.SPLIT_H, D.SPLIT_W)
    np.testing.assert_array_equal(split_rows(D.split_trajectories(), masks), gold["fg_rows"])


def test_nearest_restatement_matches_reference(gold):
    traj = torch.from_numpy(D.filter_trajectories())
    grid = torch.from_numpy(D.grid_points())
    idx = nearest(traj, grid)
    want = torch.from_numpy(gold["idx"])
    diff = (idx != want).nonzero().tolist()
    for t, g in diff:
        assert near_tie(traj[:, t], grid[g], int(idx[t, g]), int(want[t, g])), (t, g)
    print(f"near ties: {len(diff)}")
    assert len(diff) <= 8


def test_filter_restatement_matches_reference(gold):
    traj = torch.from_numpy(D.filter_trajectories())
    idx = torch.from_numpy(gold["idx"])
    gw = len(range(7, D.W, D.STRIDE))
    src, tgt = torch.from_numpy(gold["bb_source"]), torch.from_numpy(gold["bb_target"])
    off = np.concatenate([[0], np.cumsum(gold["bb_sizes"])])
    got = []
    for p, (s, t) in enumerate(gold["pairs"].tolist()):
        got.append(keep_mask(traj, idx, gw, src[off[p]:off[p + 1]], tgt[off[p]:off[p + 1]], s, t))
    np.testing.assert_array_equal(torch.cat(got).numpy(), gold["keep"])


@pytest.mark.skipif(not __import__("oracle.ref_harness", fromlist=["available"]).available(),
                    reason="no reference checkout")
def test_golden_matches_live_reference(gold):
    from oracle import ref_harness
    ref_harness.load()
    import preprocessing_dino_bb.of_filter_dino_best_buddies as OF
    import preprocessing.split_trajectories_to_fg_bg as SPLIT
    traj = torch.from_numpy(D.filter_trajectories())
    grid = torch.from_numpy(D.grid_points())
    for t in (0, D.EMPTY_FRAME, D.T - 1):
        assert torch.equal(OF.get_closest_traj_idx_batch(traj, grid, t, 30), torch.from_numpy(gold["idx"][t]))
    straj = torch.from_numpy(D.split_trajectories())
    _, first = SPLIT.generate_start_end(straj)
    np.testing.assert_array_equal(first.int().argmax(dim=1).numpy(), start_frames(straj.numpy()))
