"""CPU: the float64 oracle of the PCA foreground masks (tests/fg_mask_ref.py) equals tests/golden/fg_mask.npz, which
make_golden_fgmask.py wrote from the un-modified reference; its nearest-index rule is F.interpolate's; the checks the GPU test
uses reject planted defects; the new library entries validate their arguments without touching the device."""
import os

import numpy as np
import pytest
import torch

import fg_mask_data as D
import fg_mask_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fg_mask.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def oracle():
    return {case: R.exact_pca(np.ascontiguousarray(D.features(case).transpose(0, 2, 3, 1)), q=3) for case in D.CASES}


def signed(c0: np.ndarray, sign: int) -> np.ndarray:
    return c0 if sign > 0 else 1.0 - c0


@pytest.mark.parametrize("case", sorted(D.CASES))
def test_inputs_regenerate_bit_identically(gold, case):
    assert D.digest(D.features(case)) == str(gold[f"{case}_digest"])


@pytest.mark.parametrize("case", sorted(D.CASES))
def test_oracle_matches_reference_golden(gold, oracle, case):
    o0 = oracle[case]["colors"][..., 0]
    ref_dev = float(gold[f"{case}_ref_dev"])
    assert 0 < ref_dev < 2e-6 and float(gold[f"{case}_ratio"]) < 0.1
    sign = R.match_colors(o0, gold[f"{case}_colors0"], 4 * ref_dev, f"oracle {case}")
    assert sign == int(gold[f"{case}_sign"])
    for thr, key in zip(D.THRESHOLDS, ("tok04", "tok06")):
        assert (np.abs(o0 - thr) > 1e-4).all()                      # the generator's guarantee, both signs (0.4 and 0.6 mirror)
        np.testing.assert_array_equal(signed(o0, sign) < thr, gold[f"{case}_{key}"])
    T, _, h, w = D.CASES[case]
    H, W = D.IMG_SIZE[case]
    up = np.unpackbits(gold[f"{case}_up04"])[:T * H * W].reshape(T, H, W).astype(bool)
    np.testing.assert_array_equal(R.upsample(signed(o0, sign) < 0.4, H, W), up)


def test_reference_sign_is_not_the_truth(gold):
    """Why there is an orientation rule: the oracle's border rule puts the blob in the foreground in every case, whatever sign the
    reference's SVD returned."""
    for case in D.CASES:
        fm = np.ascontiguousarray(D.features(case).transpose(0, 2, 3, 1))
        tok = R.exact_pca(fm, q=3, orient="border")["colors"][..., 0] < 0.4
        assert tok[D.blob_tokens(case)].all() and tok.mean() < 0.5


@pytest.mark.parametrize("src,dst", [((67, 121), (476, 854)), ((11, 13), (90, 101))])
def test_nearest_rule_is_interpolate(src, dst):
    g = torch.Generator().manual_seed(5)
    tok = torch.rand((2,) + src, generator=g) < 0.5
    want = torch.nn.functional.interpolate(tok[None].float(), size=dst, mode="nearest")[0].numpy() > 0
    np.testing.assert_array_equal(R.upsample(tok.numpy(), *dst), want)


# ---- planted defects: each must fail the check the GPU test applies ------------------------------------------------------------
def test_checks_reject_a_dropped_chunk(oracle):
    o = oracle["A"]
    xc = o["xc"]
    bound = R.moments_bound(xc)
    R.check_moments((xc.T @ xc).astype(np.float32), o["cov"], bound)              # an fp32 rounding of the truth passes
    dropped = xc[:-32].T @ xc[:-32]                                               # the last stage of the last chunk missing
    with pytest.raises(AssertionError):
        R.check_moments(dropped, o["cov"], bound)


def test_checks_reject_uncentred_covariance(oracle):
    o = oracle["B"]
    rows = o["xc"] + o["mean"]
    with pytest.raises(AssertionError):
        R.check_moments(rows.T @ rows, o["cov"], R.moments_bound(o["xc"]))


def test_checks_reject_swapped_threshold_side(gold, oracle):
    o0 = oracle["A"]["colors"][..., 0]
    sign = int(gold["A_sign"])
    tol = 16 * float(gold["A_ref_dev"])
    assert R.check_mask(signed(o0, sign) < 0.4, gold["A_tok04"], signed(o0, sign), 0.4, tol) == 0
    with pytest.raises(AssertionError):
        R.check_mask(signed(o0, sign) > 0.4, gold["A_tok04"], signed(o0, sign), 0.4, tol)
    with pytest.raises(AssertionError):
        R.match_colors(o0 * 0.999, gold["A_colors0"], tol)


def test_sign_and_orientation_rules():
    V = np.array([[0.5, -0.5, 0.1], [-0.2, 0.1, 0.2], [0.1, 0.3, -0.9]])
    got = R.raw_sign(V)
    np.testing.assert_array_equal(got, np.array([[0.5, -0.5, 0.1], [0.2, -0.1, -0.2], [-0.1, -0.3, 0.9]]))
    c0 = np.full((2, 4, 5), 0.5)
    assert not R.border_flip(c0)                                   # equal means: no flip
    c0[:, 1:-1, 1:-1] = 0.9
    assert R.border_flip(c0)
    assert not R.border_flip(1.0 - c0)
    from dino_tracker_amd import fg_mask
    Vt, _ = fg_mask.principal_components(torch.diag(torch.tensor([1.0, 3.0, 2.0])), 2)
    np.testing.assert_array_equal(Vt.numpy(), np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
    assert fg_mask.border_flip(torch.from_numpy(c0)) and not fg_mask.border_flip(torch.from_numpy(1.0 - c0))


# ---- argument validation: no device needed -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle():
    import __graft_entry__ as entry
    from dino_tracker_amd import _lib
    entry.build()
    return _lib.lib()


def test_entries_validate_arguments(handle):
    one = 1   # a non-null pointer value; nothing is dereferenced on these paths
    assert handle.dtk_pca_moments(one, 100, 512, 1, 0, one, one, one, 1 << 30, None) == -1
    assert b"C must be 384, 768 or 1024" in handle.dtk_last_error()
    assert handle.dtk_pca_moments(None, 100, 384, 1, 0, one, one, one, 1 << 30, None) == -1
    assert b"null pointer" in handle.dtk_last_error()
    assert handle.dtk_pca_moments(one, 0, 384, 1, 0, one, one, one, 1 << 30, None) == -1
    assert b"bad sizes" in handle.dtk_last_error()
    assert handle.dtk_pca_moments(one, 1 << 20, 384, 1, 32, one, one, one, 1 << 30, None) == -1
    assert b"chunks" in handle.dtk_last_error()
    need = handle.dtk_pca_moments_workspace_bytes(1305, 384, 512)
    assert need >= 1305 * 4 + 3 * 384 * 384 * 4 and handle.dtk_pca_moments_workspace_bytes(1305, 500, 0) == 0
    assert handle.dtk_pca_moments(one, 1305, 384, 1, 512, one, one, one, need - 1, None) != 0
    assert b"workspace" in handle.dtk_last_error()

    assert handle.dtk_pca_project(one, 100, 500, 1, one, 3, one, one, one, 1 << 20, None) == -1
    assert b"C must be 384, 768 or 1024" in handle.dtk_last_error()
    assert handle.dtk_pca_project(one, 100, 384, 1, one, 9, one, one, one, 1 << 20, None) == -1
    assert b"q must be 1 .. 8" in handle.dtk_last_error()
    assert handle.dtk_pca_project(one, 100, 384, 1, None, 3, one, one, one, 1 << 20, None) == -1
    assert b"null pointer" in handle.dtk_last_error()
    assert handle.dtk_pca_project_workspace_bytes(100) > 0

    assert handle.dtk_fg_mask(one, 9, 0, one, 0.4, 0, 1, 2, 2, 4, 4, one, one, None) == -1
    assert b"q must be 1 .. 8" in handle.dtk_last_error()
    assert handle.dtk_fg_mask(one, 3, 3, one, 0.4, 0, 1, 2, 2, 4, 4, one, one, None) == -1
    assert handle.dtk_fg_mask(one, 3, 0, one, 0.4, 0, 1, 2, 2, 4, 4, None, one, None) == -1
    assert b"null pointer" in handle.dtk_last_error()
    assert handle.dtk_fg_mask(one, 3, 0, one, 0.4, 0, 0, 2, 2, 4, 4, one, one, None) == -1
    assert b"bad sizes" in handle.dtk_last_error()


def test_python_layer_refuses_what_it_cannot_run(handle):
    from dino_tracker_amd import fg_mask, ops
    with pytest.raises(NotImplementedError):
        fg_mask.get_fg_mask_from_pca(torch.zeros(1, 2, 2, 384), (4, 4), interpolation="bilinear")
    with pytest.raises(ValueError):
        fg_mask.get_fg_mask_from_pca(torch.zeros(1, 2, 2, 384), (4, 4), orient="up")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fg_mask.get_fg_mask_from_pca(torch.zeros(1, 2, 2, 384), (4, 4))
    with pytest.raises(RuntimeError, match="C in"):
        ops.pca_moments(torch.zeros(8, 512))


def test_all_without_make_masks_still_needs_the_reference(tmp_path):
    """`of_preprocessing all` without --make-masks: a missing mask folder is the same FileNotFoundError as before."""
    import yaml
    from dino_tracker_amd import of_preprocessing as OP
    cfg = tmp_path / "preprocessing.yaml"
    cfg.write_text(yaml.safe_dump({"video_resh": 112, "video_resw": 210, "dino_stride": 7, "fg_mask_threshold": 0.6}))
    data = tmp_path / "data"
    (data / "of_trajectories").mkdir(parents=True)
    for name in ("trajectories.pt", "trajectories_wo_direct_filter.pt"):
        torch.save(torch.zeros(1, 2, 2), data / "of_trajectories" / name)
    with pytest.raises(FileNotFoundError, match="preprocessing/create_fg_mask.py makes it"):
        OP.main(["all", "--config", str(cfg), "--data-path", str(data)])
