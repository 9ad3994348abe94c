"""Writes tests/golden/of_prep.npz by running the UN-MODIFIED reference scripts on CPU (needs a reference checkout, see oracle/ref_harness.py):
    python tests/golden/make_golden_of.py

Inputs come from tests/golden/of_prep_data.py (seeded, bit-identical everywhere; their digests are stored).  The reference runs
as is: preprocessing_dino_bb/extract_dino_best_buddies.py `run` on the seeded features, compute_dino_bb_nms.py `compute_bb_nms`
on half the pairs, of_filter_dino_best_buddies.py `run` and split_trajectories_to_fg_bg.py `mask_filter_trajectories` -- with
torch.Tensor.cuda bound to the identity for the duration of the calls (the split script calls .cuda() unconditionally).
Stored: the best-buddies input (concatenated per pair), the nearest-trajectory grids, the per-pair keep masks and the fg rows.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import ref_harness  # noqa: E402
import of_prep_data as D  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "of_prep.npz")


def main():
    ref_harness.load()   # reference + shims on sys.path (torchvision.ops for compute_dino_bb_nms)
    import preprocessing_dino_bb.extract_dino_best_buddies as BB
    import preprocessing_dino_bb.compute_dino_bb_nms as NMS
    import preprocessing_dino_bb.of_filter_dino_best_buddies as OF
    import preprocessing.split_trajectories_to_fg_bg as SPLIT
    from preprocessing_dino_bb.dino_bb_utils import create_meshgrid

    out = {}
    traj = D.filter_trajectories()
    straj = D.split_trajectories()
    out["digest_filter_traj"] = np.array(D.digest(traj))
    out["digest_split_traj"] = np.array(D.digest(straj))
    out["digest_masks"] = np.array(D.digest(D.mask_frames()))
    feats = D.bb_features()
    out["digest_features"] = np.array(D.digest(feats.numpy()))

    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with tempfile.TemporaryDirectory() as tmp:
            emb = os.path.join(tmp, "emb.pt")
            torch.save(feats, emb)
            bb_path = os.path.join(tmp, "bb", "dino_best_buddies.pt")
            BB.run(types.SimpleNamespace(dino_emb_path=emb, h=D.H, w=D.W, stride=D.STRIDE, out_path=bb_path))
            bb = torch.load(bb_path)
            coords = create_meshgrid(D.H, D.W, step=D.STRIDE)
            for key, e in bb.items():
                s, t = (int(x) for x in key.split("_"))
                if D.nms_pair(s, t):
                    NMS.compute_bb_nms(e, s, t, feats, coords, D.STRIDE, 30, 0.2)
            torch.save(bb, bb_path)

            # the nearest-trajectory grids, exactly as run() computes them
            tt = torch.from_numpy(traj)
            out["idx"] = torch.stack([OF.get_closest_traj_idx_batch(tt, coords, t, 30) for t in range(D.T)]).numpy()
            traj_path = os.path.join(tmp, "traj.pt")
            torch.save(tt, traj_path)
            filt_path = os.path.join(tmp, "bb", "filtered.pt")
            OF.run(types.SimpleNamespace(dino_bb_path=bb_path, traj_path=traj_path, out_path=filt_path,
                                         dino_bb_stride=D.STRIDE, h=D.H, w=D.W))
            filt = torch.load(filt_path)

            masks_dir = D.write_masks(os.path.join(tmp, "masks"))
            straj_path = os.path.join(tmp, "split.pt")
            torch.save(torch.from_numpy(straj), straj_path)
            fg_path, bg_path = os.path.join(tmp, "fg.pt"), os.path.join(tmp, "bg.pt")
            SPLIT.mask_filter_trajectories(straj_path, masks_dir, fg_path, filter_bg=False)
            SPLIT.mask_filter_trajectories(straj_path, masks_dir, bg_path, filter_bg=True)
            fg, bg = torch.load(fg_path), torch.load(bg_path)
    finally:
        torch.Tensor.cuda = cuda

    # best-buddies input, pairs in the reference's (s, t) order, concatenated
    pairs = [(s, t) for s in range(D.T) for t in range(D.T) if s != t]
    out["pairs"] = np.array(pairs, dtype=np.int32)
    e = [bb[f"{s}_{t}"] for s, t in pairs]
    out["bb_sizes"] = np.array([x["source_coords"].shape[0] for x in e], dtype=np.int64)
    out["bb_source"] = torch.cat([x["source_coords"] for x in e]).numpy()
    out["bb_target"] = torch.cat([x["target_coords"] for x in e]).numpy()
    out["bb_cos"] = torch.cat([x["cos_sims"] for x in e]).numpy()
    out["bb_nms"] = np.array([D.nms_pair(s, t) for s, t in pairs])
    out["bb_peak_affs"] = torch.cat([x["peak_affs"] for x, m in zip(e, out["bb_nms"]) if m]).numpy()
    out["bb_r"] = torch.cat([x["r"] for x, m in zip(e, out["bb_nms"]) if m]).numpy()

    # filter: keep mask per entry, recovered from the reference's filtered coordinates (every kept row is a row of the input;
    # one pair's buddies have distinct source cells, so the source coordinate identifies the row)
    keep = []
    for (s, t), x in zip(pairs, e):
        f = filt[f"{s}_{t}"]
        k = np.zeros(x["source_coords"].shape[0], dtype=bool)
        if f["source_coords"] is not None:
            src = x["source_coords"]
            hit = (src[:, None, :] == f["source_coords"][None, :, :]).all(-1)
            assert (hit.sum(0) == 1).all()
            k = hit.any(1).numpy()
            assert torch.equal(src[k], f["source_coords"]) and torch.equal(x["target_coords"][k], f["target_coords"])
            assert torch.equal(x["cos_sims"][k], f["cos_sims"])
            if D.nms_pair(s, t):
                assert torch.equal(x["peak_affs"][k], f["peak_affs"]) and torch.equal(x["r"][k], f["r"])
            else:
                assert f["peak_affs"] is None and f["r"] is None
        else:
            assert all(f[n] is None for n in ("target_coords", "cos_sims", "peak_coords", "peak_affs", "r"))
        keep.append(k)
    out["keep"] = np.concatenate(keep)

    # split: fg / bg row indices -- fg and bg partition the input in order (boolean indexing), so a merge recovers the rows
    st = torch.from_numpy(straj)
    nan_eq = lambda a, b: bool(((a == b) | (a.isnan() & b.isnan())).all())  # noqa: E731
    isfg = np.zeros(st.shape[0], dtype=bool)
    i = 0
    for n in range(st.shape[0]):
        if i < fg.shape[0] and nan_eq(st[n], fg[i]):
            isfg[n] = True
            i += 1
    assert nan_eq(st[torch.from_numpy(isfg)], fg) and nan_eq(st[torch.from_numpy(~isfg)], bg)
    out["fg_rows"] = np.nonzero(isfg)[0].astype(np.int32)

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT} ({size / 1024:.0f} KiB): {int(out['bb_sizes'].sum())} buddies, {int(out['keep'].sum())} kept, "
          f"{len(out['fg_rows'])} fg of {straj.shape[0]}")
    assert size < 1 << 20


if __name__ == "__main__":
    main()
