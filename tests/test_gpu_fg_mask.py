"""GPU: the PCA foreground masks (csrc/pca.hip, dino_tracker_amd/fg_mask.py) against the float64 oracle of tests/fg_mask_ref.py
and the reference golden tests/golden/fg_mask.npz (make_golden_fgmask.py).  Bounds and what they cover: fg_mask_ref.py."""
import os

import numpy as np
import pytest
import torch

import fg_mask_data as D
import fg_mask_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fg_mask.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def maps():
    """case -> feature map [T, h, w, C] float32 (numpy), the layout get_fg_mask_from_pca takes."""
    return {case: np.ascontiguousarray(D.features(case).transpose(0, 2, 3, 1)) for case in D.CASES}


@pytest.fixture(scope="module")
def oracle(maps):
    return {case: R.exact_pca(maps[case], q=3) for case in D.CASES}


def big_rows(C: int) -> np.ndarray:
    """T = 2 frames of 67 x 121 tokens: [16214, C] float32, a shared offset, a blob direction on a fifth of the rows, noise."""
    g = torch.Generator().manual_seed(67121 + C)
    n = 2 * 67 * 121
    x = torch.randn(n, C, generator=g) * 0.5 + torch.randn(C, generator=g)[None] * 1.5
    x[: n // 5] += torch.randn(C, generator=g)[None]
    return x.numpy()


# ---- 1. moments, exact class ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [384, 1024])
@pytest.mark.parametrize("N,chunk_rows", [(1305, 512), (286, 0)])
def test_moments_exact_integers(N, chunk_rows, C):
    """Small integers in +- pairs (every column sums to 0, so the mean is exactly 0 and centring changes nothing): every
    product and every partial sum is an integer below 2^24, so any summation order is exact and cov must be bit-equal to
    the integer Gram.  N = 1305 with chunk_rows = 512 is three uneven chunks with a ragged last stage."""
    from dino_tracker_amd import ops
    rng = np.random.default_rng(N + C)
    half = rng.integers(-3, 4, size=(N // 2, C))
    x = np.concatenate([half, -half, np.zeros((N % 2, C), dtype=half.dtype)])
    x = x[rng.permutation(N)]
    want = (x.T @ x).astype(np.float32)
    assert np.abs(x.T @ x).max() < 2 ** 24
    mean, cov = ops.pca_moments(torch.from_numpy(x.astype(np.float32)).to(DEV), normalize=False, chunk_rows=chunk_rows)
    mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
    assert (mean == 0).all()
    print(f"exact N={N} C={C}: {int((cov != want).sum())} of {cov.size} elements differ, max |diff| {np.abs(cov - want).max()}")
    np.testing.assert_array_equal(cov, want)
    np.testing.assert_array_equal(cov, cov.T)


# ---- 2. moments, realistic ------------------------------------------------------------------------------------------------
def _moments_case(name, maps):
    if name in D.CASES:
        fm = maps[name]
        return fm.reshape(-1, fm.shape[-1])
    return big_rows(int(name[3:]))


@pytest.mark.parametrize("name", ["A", "B", "C", "big384", "big1024"])
def test_moments_realistic(name, maps):
    from dino_tracker_amd import ops
    x = _moments_case(name, maps)
    N = x.shape[0]
    rows = R.rows_of(x)
    mean, cov, xc = R.moments(rows)
    bound = R.moments_bound(xc)
    xd = torch.from_numpy(x).to(DEV)
    small = 96 if N < 2000 else 1024
    m1, c1 = ops.pca_moments(xd)
    m2, c2 = ops.pca_moments(xd)
    m3, c3 = ops.pca_moments(xd, chunk_rows=small)
    assert torch.equal(c1, c2) and torch.equal(m1, m2)                     # fixed reduction order: the same bits
    c1n, c3n = c1.cpu().numpy(), c3.cpu().numpy()
    print(f"{name}: N={N} max |mean err| {np.abs(m1.cpu().numpy() - mean).max():.3e}")
    assert np.abs(m1.cpu().numpy() - mean).max() <= 2.0 ** -22             # a few fp32 roundings of values below 1
    R.check_moments(c1n, cov, bound, f"{name} default chunks")
    R.check_moments(c3n, cov, bound, f"{name} chunk_rows={small}")
    R.check_moments(c3n, c1n.astype(np.float64), bound, f"{name} default vs chunk_rows={small}")
    np.testing.assert_array_equal(c1n, c1n.T)
    np.testing.assert_array_equal(c3n, c3n.T)


@pytest.mark.parametrize("case", ["B", "C"])
def test_project_eight_components(case, maps):
    """q = 8 (the most the entry takes), C = 1024 / 768: colours against float64, min / max exactly those of the colours."""
    from dino_tracker_amd import ops
    fm = maps[case]
    x = fm.reshape(-1, fm.shape[-1])
    V = torch.randn(8, x.shape[1], generator=torch.Generator().manual_seed(8)) / x.shape[1] ** 0.5
    colors, minmax = ops.pca_project(torch.from_numpy(x).to(DEV), V.to(DEV))
    want = R.rows_of(x) @ V.double().numpy().T
    err = np.abs(colors.cpu().numpy() - want).max()
    print(f"project {case}: max |err| {err:.3e}")
    # fp32 dot of a unit row (C terms, |row| |V_j| <= ~1.2): C 2^-24 worst case, far less in practice
    assert err <= x.shape[1] * 2.0 ** -24 * 1.5
    assert torch.equal(minmax[:8], colors.min(dim=0).values) and torch.equal(minmax[8:], colors.max(dim=0).values)


# ---- 3. colours and masks against the reference golden -------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(D.CASES))
def test_colors_and_masks_match_reference(case, maps, oracle, gold):
    from dino_tracker_amd import fg_mask
    fm = torch.from_numpy(maps[case]).to(DEV)
    T, _, h, w = D.CASES[case]
    H, W = D.IMG_SIZE[case]
    tol_c = 16 * float(gold[f"{case}_ref_dev"])
    gold_c0 = gold[f"{case}_colors0"]
    _, det = fg_mask.get_fg_mask_from_pca(fm, (H, W), orient="positive", return_details=True)
    sign = R.match_colors(det["colors"][..., 0].cpu().numpy(), gold_c0, tol_c, f"{case} positive")
    assert sign == int(gold[f"{case}_sign"])                               # the raw sign rule is the oracle's
    o0 = oracle[case]["colors"][..., 0]
    o0 = o0 if sign > 0 else 1.0 - o0                                      # float64 colours in the reference's sign
    ups = np.unpackbits(gold[f"{case}_up04"])[:T * H * W].reshape(T, H, W).astype(bool)
    for thr, key in zip(D.THRESHOLDS, ("tok04", "tok06")):
        # the mask of the reference's sign: `invert` is the override that selects it
        out, det = fg_mask.get_fg_mask_from_pca(fm, (H, W), fg_mask_threshold=thr, orient="positive", invert=sign < 0,
                                                return_details=True)
        assert R.match_colors(det["colors"][..., 0].cpu().numpy(), gold_c0, tol_c, f"{case} reference sign") == 1
        tok = det["token_mask"].cpu().numpy()
        assert set(np.unique(tok)) <= {0, 255} and tok.shape == (T, h, w)
        R.check_mask(tok, gold[f"{case}_{key}"], o0, thr, tol_c, what=f"{case} token mask")
        mask = det["mask"].cpu().numpy()
        np.testing.assert_array_equal(mask, R.upsample(tok, H, W))
        assert out.dtype == np.float32 and out.shape == (T, H, W)
        np.testing.assert_array_equal(out, (mask > 0).astype(np.float32))
        if thr == 0.4 and ((tok > 0) == gold[f"{case}_{key}"]).all():
            np.testing.assert_array_equal(mask > 0, ups)


# ---- 4. orientation ---------------------------------------------------------------------------------------------------------
def test_orientation_rules(maps, gold):
    from dino_tracker_amd import fg_mask
    fm = torch.from_numpy(maps["A"]).to(DEV)
    H, W = D.IMG_SIZE["A"]
    tol_c = 16 * float(gold["A_ref_dev"])
    _, b = fg_mask.get_fg_mask_from_pca(fm, (H, W), return_details=True)               # orient="border" is the default
    tok = b["token_mask"].cpu().numpy() > 0
    assert tok[D.blob_tokens("A")].all() and tok.mean() < 0.5
    _, bn = fg_mask.get_fg_mask_from_pca(-fm, (H, W), return_details=True)
    assert torch.equal(bn["mask"], b["mask"]) and bn["flipped"] != b["flipped"]
    _, p = fg_mask.get_fg_mask_from_pca(fm, (H, W), orient="positive", return_details=True)
    _, pn = fg_mask.get_fg_mask_from_pca(-fm, (H, W), orient="positive", return_details=True)
    assert not p["flipped"] and not pn["flipped"]
    mirror = (pn["colors"][..., 0] - (1.0 - p["colors"][..., 0])).abs().max().item()
    print(f"negated features: max |c' - (1 - c)| {mirror:.3e}")
    assert mirror <= tol_c
    # invert thresholds 1 - c: at 0.4 that is the mask of the mirrored colours, and at 0.5 the complement except where c == 0.5
    _, pi = fg_mask.get_fg_mask_from_pca(fm, (H, W), orient="positive", invert=True, return_details=True)
    assert pi["flipped"] and torch.equal(pi["colors"][..., 0], 1.0 - p["colors"][..., 0])
    assert torch.equal(pi["token_mask"] > 0, pi["colors"][..., 0] < 0.4)
    _, h0 = fg_mask.get_fg_mask_from_pca(fm, (H, W), fg_mask_threshold=0.5, orient="positive", return_details=True)
    _, h1 = fg_mask.get_fg_mask_from_pca(fm, (H, W), fg_mask_threshold=0.5, orient="positive", invert=True, return_details=True)
    off_thr = h0["colors"][..., 0] != 0.5
    assert torch.equal((h1["token_mask"] > 0)[off_thr], ~(h0["token_mask"] > 0)[off_thr])
    assert 0 < int((h0["token_mask"] > 0).sum()) < h0["token_mask"].numel()


# ---- 5. upsampling and degenerate input -------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(476, 854), (480, 854)])
def test_upsampling_is_interpolate_nearest(size):
    from dino_tracker_amd import ops
    T, h, w = 2, 67, 121
    g = torch.Generator().manual_seed(size[0])
    colors = (torch.rand(T * h * w, 3, generator=g) < 0.5).float()
    minmax = torch.zeros(16)
    minmax[8:] = 1.0
    for comp, flip in ((0, False), (2, True)):
        mask, tok = ops.fg_mask(colors.to(DEV), minmax.to(DEV), (T, h, w), size, 0.5, comp=comp, flip=flip)
        want_tok = (colors[:, comp] < 0.5) != flip
        assert torch.equal(tok.cpu() > 0, want_tok.reshape(T, h, w))
        want = torch.nn.functional.interpolate(want_tok.reshape(1, T, h, w).float(), size=size, mode="nearest")[0]
        assert torch.equal(mask.cpu(), (want * 255).to(torch.uint8))


def test_constant_colors_give_an_empty_mask():
    from dino_tracker_amd import ops
    T, h, w = 1, 5, 7
    colors = torch.full((T * h * w, 2), 0.25, device=DEV)
    minmax = torch.full((16,), 0.25, device=DEV)
    for flip in (False, True):
        mask, tok = ops.fg_mask(colors, minmax, (T, h, w), (20, 30), 0.4, flip=flip)      # 0 / 0 compares false
        assert int(mask.max()) == 0 and int(tok.max()) == 0


# ---- 6. paths ---------------------------------------------------------------------------------------------------------------
def test_video_path_equals_feature_path():
    from dino_tracker_amd import fg_mask, ops, synth
    from dino_tracker_amd.extractor import VitExtractor
    sd = synth.make_vit_weights("dinov2_vits14", seed=2, layerscale=0.1)
    video = synth.synth_video(3, 112, 210, seed=71)
    ex = VitExtractor("dinov2_vits14", stride=7, device=DEV, state_dict=sd)
    _, a = fg_mask.fg_masks_from_video(video, "dinov2_vits14", layer=3, stride=7, extractor=ex, frame_batch=3, return_details=True)
    feat = ex.encode(video, layer=3)                                                     # [3, 15 * 29, 384] on the device
    assert a["mask"].shape == (3, 112, 210) and a["token_mask"].shape == (3, 15, 29)
    _, b = fg_mask.fg_masks_from_features(feat, (112, 210), grid=(15, 29), return_details=True)
    _, c = fg_mask.fg_masks_from_features(ops.unpack_features(feat, 15, 29).cpu(), (112, 210), return_details=True)
    for other in (b, c):
        assert torch.equal(a["mask"], other["mask"]) and torch.equal(a["colors"], other["colors"])
    assert 0 < int((a["token_mask"] > 0).sum()) < a["token_mask"].numel()


def test_command_lines(tmp_path, maps):
    import yaml
    from dino_tracker_amd import fg_mask, of_preprocessing as OP
    from dino_tracker_amd.train import load_masks
    T, C, h, w = D.CASES["A"]
    H, W = D.IMG_SIZE["A"]
    feats = torch.from_numpy(D.features("A"))
    data = tmp_path / "data"
    (data / "dino_embeddings").mkdir(parents=True)
    emb = data / "dino_embeddings" / "dino_embed_video-layer=23.pt"
    torch.save(feats, emb)
    fg_mask.main(["--dino-embed-video-path", str(emb), "--h", str(H), "--w", str(W), "--mask-path", str(tmp_path / "m"),
                  "--fg_mask_threshold", "0.4", "--orient", "positive", "--invert"])
    files = sorted(os.listdir(tmp_path / "m"))
    assert files == [f"{t:05d}.png" for t in range(T)]
    _, det = fg_mask.fg_masks_from_features(feats, (H, W), orient="positive", invert=True, return_details=True)
    assert torch.equal(load_masks(str(tmp_path / "m"), H, W), det["mask"].cpu())

    cfg = tmp_path / "preprocessing.yaml"
    cfg.write_text(yaml.safe_dump({"video_resh": H, "video_resw": W, "dino_stride": 7, "fg_mask_threshold": 0.6}))
    OP.main(["masks", "--config", str(cfg), "--data-path", str(data)])
    _, det = fg_mask.fg_masks_from_features(feats, (H, W), fg_mask_threshold=0.6, return_details=True)
    assert torch.equal(load_masks(str(data / "masks"), H, W), det["mask"].cpu())

    # `all` without --make-masks: a missing mask folder is still the reference's job
    other = tmp_path / "other"
    (other / "of_trajectories").mkdir(parents=True)
    for name in ("trajectories.pt", "trajectories_wo_direct_filter.pt"):
        torch.save(torch.zeros(1, 2, 2), other / "of_trajectories" / name)
    with pytest.raises(FileNotFoundError, match="preprocessing/create_fg_mask.py makes it"):
        OP.main(["all", "--config", str(cfg), "--data-path", str(other)])
