"""Seeded inputs of the CPU unit tests that pin the oracle and the trainer against the reference
(tests/test_oracle_vs_reference.py, tests/test_trainer_vs_reference.py, tests/test_train_vs_reference.py), and the reference's side of each comparison.  make_golden.py runs `reference_values()` on the UN-MODIFIED reference and stores the
result as tests/golden/ref_units.npz; the tests rebuild the same inputs here and compare against the stored values, so they
need no reference checkout."""
import numpy as np
import torch

from dino_tracker_amd import synth
from oracle import ref_algo as A

GOLDEN = "ref_units.npz"


def delta_dino_case():
    c = 24
    return c, synth.synth_delta_dino_weights(c, seed=7), synth.synth_video(2, 98, 126, seed=5), torch.zeros(2, c, 13, 17)


def tracker_forward_case():
    H, W, T, C = 112, 154, 5, 16
    ph, pw = A.feature_grid(H, W)
    video = synth.synth_video(T, H, W, seed=21)
    feats = synth.synth_features(T, C, ph, pw, seed=22)
    head = synth.synth_head_weights(23)
    pts = torch.tensor([[30.0, 40.0, 1.0], [100.5, 77.25, 3.0], [2.0, 3.0, 0.0], [150.0, 110.0, 4.0]])
    tgt = torch.tensor([4, 0, 2, 2])
    return H, W, T, video, feats, head, pts, tgt


def tapvid_case():
    """A metrics config of three query frames on random tracks with realistic error scales; predictions at 854 x 476."""
    g = np.random.default_rng(0)
    T = 9
    cfg = {"video_idx": 3, "h": 256, "w": 256, "query_points": {}, "target_points": {}, "occluded": {}}
    preds = {}
    for f, n in ((0, 5), (4, 7), (8, 3)):
        gt = g.uniform(0, 255, (n, T, 2)).astype(np.float32)
        occ = g.uniform(size=(n, T)) < 0.3
        noise = g.normal(size=(n, T, 2)) * g.choice([0.3, 1.5, 6.0, 30.0], size=(n, T, 1))
        pred = ((gt + noise) * np.array([854 / 256, 476 / 256])).astype(np.float32)
        pocc = occ ^ (g.uniform(size=(n, T)) < 0.2)
        cfg["query_points"][f] = gt[:, f].tolist()
        cfg["target_points"][f], cfg["occluded"][f] = gt, occ
        preds[f] = (pred, pocc)
    return cfg, preds


def best_buddies_case():
    T, C, Hh, Ww = 3, 16, 98, 126
    return T, Hh, Ww, synth.synth_features(T, C, 13, 17, seed=33)


def bb_nms_case():
    """Best buddies of every frame pair of a smooth random feature field (33 x 45 cells), from the oracle."""
    from dino_tracker_amd.best_buddies import create_meshgrid
    T, C, Hh, Ww = 3, 32, 238, 322
    ph, pw = 33, 45
    feats = synth.synth_features(T, C, ph, pw, seed=35)
    coords = create_meshgrid(Hh, Ww)
    tm = feats.permute(0, 2, 3, 1).reshape(T, -1, C)
    bbs = {}
    for s in range(T):
        for t in range(T):
            if s != t:
                si, ti, cs = A.best_buddies_pair(tm[s], tm[t])
                bbs[f"{s}_{t}"] = {"source_coords": coords[si], "target_coords": coords[ti], "cos_sims": cs}
    return T, ph, pw, feats, coords, tm, bbs


BB_NMS_PAIRS = ((0, 1), (0, 2), (1, 2))


def reference_values(R, tmp):
    """The reference's outputs on the inputs above.  R: oracle.ref_harness.load(); tmp: a scratch directory."""
    import os
    import types
    out = {}
    c, sd, frames, vit = delta_dino_case()
    net = R.delta_dino.DeltaDINO(channels=[3, 64, 128, 256, c], vit_stride=7).eval()
    net.load_state_dict(sd)
    with torch.no_grad():
        out["delta_dino"] = net(frames, vit).numpy()

    H, W, T, video, feats, head, pts, tgt = tracker_forward_case()
    torch.save(feats, os.path.join(tmp, "e.pt"))
    trk = R.tracker.Tracker(video=video, ckpt_path=tmp, dino_embed_path=os.path.join(tmp, "e.pt"), device="cpu")
    trk.tracker_head.load_state_dict(head)
    with torch.no_grad():
        out["tracker_forward"] = trk((pts, pts[:, 2].long(), tgt, torch.arange(T).int()), use_raw_features=True).numpy()

    import eval.metrics as EM
    cfg, preds = tapvid_case()
    d = os.path.join(tmp, "tapvid")
    os.makedirs(d)
    for f, (pred, pocc) in preds.items():
        np.save(os.path.join(d, f"trajectories_{f}.npy"), pred)
        np.save(os.path.join(d, f"occlusion_preds_{f}.npy"), pocc)
    want = EM.compute_tapvid_metrics_for_video(d, d, {"videos": [cfg]}, 3, pred_video_sizes=[854, 476])
    out["tapvid_names"] = np.array(sorted(want))
    out["tapvid_values"] = np.array([float(want[k]) for k in sorted(want)], dtype=np.float64)

    import preprocessing_dino_bb.extract_dino_best_buddies as BB
    T, Hh, Ww, feats = best_buddies_case()
    torch.save(feats, os.path.join(tmp, "emb.pt"))
    bb_path = os.path.join(tmp, "bb", "bb.pt")
    BB.run(types.SimpleNamespace(dino_emb_path=os.path.join(tmp, "emb.pt"), h=Hh, w=Ww, stride=7, out_path=bb_path))
    bb = torch.load(bb_path)
    out["bb_pairs"] = np.array(sorted(bb))
    for k, e in bb.items():
        for f in ("source_coords", "target_coords", "cos_sims"):
            out[f"bb_{k}_{f}"] = e[f].cpu().numpy()

    import preprocessing_dino_bb.compute_dino_bb_nms as NMS
    T, ph, pw, feats, coords, tm, bbs = bb_nms_case()
    for (s, t) in BB_NMS_PAIRS:
        want = {}
        for a, b in ((s, t), (t, s)):
            e = {k: v.clone() for k, v in bbs[f"{a}_{b}"].items()}
            want[(a, b)] = NMS.compute_bb_nms(e, a, b, feats, coords, 7, 50, 0.2)
            out[f"nms_{a}_{b}_peak_affs"] = want[(a, b)]["peak_affs"].clone().numpy()   # (before compute_max_r sees them)
            out[f"nms_{a}_{b}_r"] = want[(a, b)]["r"].clone().numpy()
        m, mr = NMS.compute_max_r(want[(s, t)], want[(t, s)])
        out[f"max_r_{s}_{t}"] = m["r"].numpy()
        out[f"max_r_{t}_{s}"] = mr["r"].numpy()
    out.update(trainer_reference_values(R))
    out.update(train_reference_values(R))
    return {k: np.array(v, copy=True) for k, v in out.items()}


# ---- tests/test_trainer_vs_reference.py: the loss terms of the reference's trainer (dino_tracker.py) ---------------------
TRAINER_CONFIG = {
    "cl_n_frames": 4, "cl_points_per_pair": 40, "cl_fg_points_ratio": 0.7, "cl_temp": 0.1, "cl_div_dino_bb": 700,
    "cl_div_ref_bb": 900, "bb_amb_sig_a": 27, "bb_amb_sig_b": -5.7, "dino_patch_size": 14, "cyc_gamma": 0.8,
    "lambda_cyc": 0.5, "lambda_cl_ref_bb": 5e-5, "lambda_cl_dino_bb": 2.5e-4, "lambda_emb_norm": 1e-4, "lambda_angle": 1e-4,
}
TRAINER_H, TRAINER_W, TRAINER_FRAMES, TRAINER_C = 126, 182, 6, 16


def trainer_scene():
    """Masks, best buddies of every frame pair (some empty or None), the batch's frame set and embeddings."""
    H, W, FRAMES, C = TRAINER_H, TRAINER_W, TRAINER_FRAMES, TRAINER_C
    g = torch.Generator().manual_seed(0)
    h, w = (H - 14) // 7 + 1, (W - 14) // 7 + 1
    fg_masks = torch.zeros(FRAMES, H, W)
    for f in range(FRAMES):
        fg_masks[f, 20 + 3 * f:90, 30:120 + 5 * f] = 1.0
    pairs = {}
    for s in range(FRAMES):
        for t in range(FRAMES):
            if s == t:
                continue
            n = int(torch.randint(0, 90, (1,), generator=g)) if (s + t) % 5 else 0
            if n == 0:
                pairs[f"{s}_{t}"] = {"source_coords": None if s % 2 else torch.zeros(0, 2), "target_coords": None,
                                     "cos_sims": None, "r": None}
                continue
            xy = lambda: torch.stack([torch.rand(n, generator=g) * (W - 15) + 7, torch.rand(n, generator=g) * (H - 15) + 7], 1)  # noqa: E731
            pairs[f"{s}_{t}"] = {"source_coords": xy(), "target_coords": xy(), "cos_sims": torch.rand(n, generator=g) * 1.2 - 0.2,
                                 "r": torch.rand(n, generator=g)}
    frames_set_t = torch.tensor([0, 2, 3, 5], dtype=torch.int32)
    emb = torch.randn(4, C, h, w, generator=g) + 0.3
    raw = emb + 0.1 * torch.randn(4, C, h, w, generator=g)
    return fg_masks, pairs, frames_set_t, emb, raw, h, w


def trainer_model_like(tracker_cls, emb, raw):
    """A stand-in model holding the batch's embeddings, with the two sampling methods of `tracker_cls`."""
    import types
    m = types.SimpleNamespace()
    m.video = torch.zeros(TRAINER_FRAMES, 3, TRAINER_H, TRAINER_W)
    m.dino_patch_size, m.stride, m.device = 14, 7, "cpu"
    m.frame_embeddings = emb.clone().requires_grad_(True)
    m.raw_embeddings = raw
    m._refined = m._dino = None
    m.normalize_points_for_sampling = types.MethodType(tracker_cls.normalize_points_for_sampling, m)
    m.sample_embeddings = types.MethodType(tracker_cls.sample_embeddings, m)
    return m


def cycle_case():
    g = torch.Generator().manual_seed(6)
    x, y = torch.randn(50, 2, generator=g) * 0.05, torch.randn(50, 2, generator=g) * 0.05
    keep = torch.rand(50, generator=g) > 0.4
    preds = {"source_coords": torch.randn(50, 3, generator=g), "target_coords": torch.randn(50, 3, generator=g),
             "source_target_coords": torch.randn(50, 2, generator=g), "target_source_coords": torch.randn(50, 2, generator=g),
             "cycle_consistency_dists": torch.rand(50, generator=g) * 4}
    return x, y, keep, preds


def _recorded(fn):
    """fn() with what torch.randint / torch.randperm return recorded: (result, randint draws, randperm draws)."""
    ri, rp = torch.randint, torch.randperm
    rec_i, rec_p = [], []

    def randint(*a, **k):
        out = ri(*a, **k)
        rec_i.append(out.clone())
        return out

    def randperm(*a, **k):
        out = rp(*a, **k)
        rec_p.append(out.clone())
        return out
    torch.randint, torch.randperm = randint, randperm
    try:
        return fn(), rec_i, rec_p
    finally:
        torch.randint, torch.randperm = ri, rp


def _ragged(prefix, rows):
    return {f"{prefix}_cat": torch.cat(rows).numpy() if rows else np.zeros(0, np.int64),
            f"{prefix}_len": np.array([len(r) for r in rows], dtype=np.int64)}


def unragged(gold, prefix):
    cat, lens = torch.from_numpy(gold[f"{prefix}_cat"]), gold[f"{prefix}_len"].tolist()
    return list(torch.split(cat, lens)) if lens else []


def trainer_reference_values(R):
    """The reference trainer's loss terms on trainer_scene(): values, gradients with respect to the frame embeddings, the
    random draws the terms made, and the foreground flags of models/utils.filter_bb_foreground_pairs per frame pair."""
    import types
    import models.utils as mu
    import dino_tracker as ref_dt
    cuda, defaults = torch.Tensor.cuda, mu.get_vit_feature_coords_from_mask.__defaults__
    torch.Tensor.cuda = lambda self, *a, **k: self
    mu.get_vit_feature_coords_from_mask.__defaults__ = (7, 14, "cpu")
    try:
        fg_masks, pairs, frames_set_t, emb, raw, h, w = trainer_scene()
        theirs = object.__new__(ref_dt.DINOTracker)
        theirs.config, theirs.fg_masks, theirs.dino_bb_pairs = dict(TRAINER_CONFIG), fg_masks, pairs
        theirs.of_loss_fn = torch.nn.HuberLoss(delta=1 / 32, reduction="none")
        out = {}
        for s in range(TRAINER_FRAMES):
            for t in range(TRAINER_FRAMES):
                bb = pairs.get(f"{s}_{t}")
                if bb is not None and bb["source_coords"] is not None and bb["source_coords"].shape[0] > 0:
                    _, _, fg = mu.filter_bb_foreground_pairs(bb["source_coords"], bb["target_coords"], fg_masks[s],
                                                             resw=TRAINER_W, resh=TRAINER_H)
                    out[f"trainer_fg_{s}_{t}"] = fg.numpy()
        for tag, seed, method in (("dino_bb", 3, theirs.get_dino_bb_contrastive_loss),
                                  ("refined_bb", 4, theirs.get_refiner_contrastive_loss)):
            m = trainer_model_like(R.tracker.Tracker, emb, raw)
            torch.manual_seed(seed)
            want, rec_i, rec_p = _recorded(lambda: method(m, frames_set_t))
            want.backward()
            out[f"trainer_{tag}_value"] = np.array(float(want), dtype=np.float64)
            out[f"trainer_{tag}_grad"] = m.frame_embeddings.grad.numpy()
            out.update(_ragged(f"trainer_{tag}_randint", rec_i))
            out.update(_ragged(f"trainer_{tag}_randperm", rec_p))
        m = trainer_model_like(R.tracker.Tracker, emb, raw)
        out["trainer_emb_norm"] = np.array(float(theirs.get_emb_norm_regularization_loss(m)), dtype=np.float64)
        out["trainer_emb_angle"] = np.array(float(theirs.get_emb_angle_regularization_loss(m)), dtype=np.float64)
        x, y, keep, preds = cycle_case()
        out["trainer_huber_mean"] = np.array(float(theirs.of_loss_fn(x, y).mean()), dtype=np.float64)
        kept = {k: v[keep] for k, v in preds.items()}
        m_t = types.SimpleNamespace(get_cycle_consistent_preds=lambda frames, masks: kept)
        out["trainer_cycle"] = np.array(float(theirs.get_cycle_consistency_loss(m_t, (None, frames_set_t))), dtype=np.float64)
        return out
    finally:
        torch.Tensor.cuda = cuda
        mu.get_vit_feature_coords_from_mask.__defaults__ = defaults


# ---- tests/test_train_vs_reference.py: alignment matrices, config/train.yaml, trajectory sampler draws ---------------------
def align_cases():
    g = torch.Generator().manual_seed(2)
    return [(torch.randn(2, 5, hc, wc, generator=g), h, w) for (hc, wc, h, w) in ((60, 107, 67, 121), (9, 13, 9, 13), (16, 107, 17, 121))]


def sampler_case():
    g = torch.Generator().manual_seed(4)
    T, W, H = 12, 210, 126

    def trajectories(n):
        tr = torch.rand(n, T, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
        tr[torch.rand(n, T, generator=g) < 0.45] = float("nan")
        return tr
    fg, bg = trajectories(300), trajectories(500)
    return T, W, H, fg, bg, dict(batch_size=64, dst_range=(-1, 1), fg_traj_ratio=0.5, num_frames=4, keep_in_cpu=False)


SAMPLER_SEEDS = range(5)


def yaml_digest(cfg):
    """sha256 of a parsed YAML document in canonical JSON form."""
    import hashlib
    import json
    return hashlib.sha256(json.dumps(cfg, sort_keys=True).encode()).hexdigest()


def train_reference_values(R):
    import os
    import yaml
    from oracle import ref_harness
    out = {}
    for i, (cnn, h, w) in enumerate(align_cases()):
        out[f"train_align_{i}"] = R.models_utils.align_cnn_vit_features(torch.zeros(2, 5, h, w), cnn, cnn_stride=8, vit_stride=7).numpy()
    with open(os.path.join(ref_harness.REFERENCE_ROOT, "config", "train.yaml")) as fh:
        out["train_yaml_sha256"] = np.array(yaml_digest(yaml.safe_load(fh.read())))
    T, W, H, fg, bg, kw = sampler_case()
    theirs = R.dataset.DinoTrackerSampler(range_normalizer=R.dataset.RangeNormalizer(shapes=(W, H, T)), fg_trajectories=fg.clone(),
                                          bg_trajectories=bg.clone(), **kw)
    for seed in SAMPLER_SEEDS:
        torch.manual_seed(seed)
        a = theirs()
        out[f"train_sampler_{seed}_keys"] = np.array(list(a))
        for k, v in a.items():
            out[f"train_sampler_{seed}_{k}"] = v.numpy()
    return out
