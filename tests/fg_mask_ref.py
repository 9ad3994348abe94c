"""The float64 oracle of the PCA foreground masks and the checks the CPU and GPU tests share.

Oracle: F.normalize, centre, `eigh` of the centred covariance, project the UNCENTRED rows, min-max, the sign and orientation
rules of dino_tracker_amd/fg_mask.py, nearest-neighbour source indices.  Everything in numpy float64.

Checks (used on device results by tests/test_gpu_fg_mask.py and on planted defects by tests/test_fg_mask_reference.py):
  check_moments -- per element |got - ref| <= (2^-21 + 2 N 2^-24) (|Xc|^T |Xc|): the first term covers the hi + lo fp16 planes
                   (2^-22 per operand, twice) and the dropped lo.lo product, the second the worst-case fp32 sum of N terms
                   with two roundings per term (the argument of tests/vit_gemm_ref.py class (b)).
  match_colors  -- normalised component-0 colours equal the golden's or one minus them within a tolerance; returns the sign.
  check_mask    -- token masks equal, except on tokens whose float64 colour is within the tolerance of the threshold (few).
"""
import numpy as np

EPS_NORM = 1e-12


def normalize_rows(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.float64)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), EPS_NORM)


def rows_of(feature_map: np.ndarray, normalize: bool = True) -> np.ndarray:
    """[..., C] -> float64 rows [N, C], normalised as F.normalize does."""
    x = feature_map.reshape(-1, feature_map.shape[-1]).astype(np.float64)
    return normalize_rows(x) if normalize else x


def moments(rows: np.ndarray):
    """(mean [C], cov [C, C] = Xc^T Xc, Xc) of float64 rows."""
    mean = rows.mean(axis=0)
    xc = rows - mean
    return mean, xc.T @ xc, xc


def moments_bound(xc: np.ndarray) -> np.ndarray:
    n = xc.shape[0]
    a = np.abs(xc)
    return (2.0 ** -21 + 2.0 * n * 2.0 ** -24) * (a.T @ a)


def raw_sign(V: np.ndarray) -> np.ndarray:
    """rows = eigenvectors: the largest-magnitude entry of each positive, the lowest index on ties."""
    lead = V[np.arange(V.shape[0]), np.abs(V).argmax(axis=1)]
    return np.where(lead[:, None] < 0, -V, V)


def components(cov: np.ndarray, q: int):
    """(V [q, C] with the raw sign rule, all eigenvalues descending)."""
    w, v = np.linalg.eigh(cov)
    return raw_sign(v[:, ::-1][:, :q].T.copy()), w[::-1]


def min_max(colors: np.ndarray) -> np.ndarray:
    mn, mx = colors.min(axis=0), colors.max(axis=0)
    return (colors - mn) / (mx - mn)


def border_flip(c0: np.ndarray) -> bool:
    """c0 [T, h, w] normalised component 0: flip when the outermost ring of the grid is, on average, below all tokens."""
    ring = np.zeros(c0.shape[1:], dtype=bool)
    ring[0, :] = ring[-1, :] = True
    ring[:, 0] = ring[:, -1] = True
    return bool(c0[:, ring].mean() < c0.mean())


def exact_pca(feature_map: np.ndarray, q: int = 3, normalize: bool = True, orient: str = "positive", invert: bool = False):
    """feature_map [T, h, w, C] -> dict(mean, cov, xc, evals, V, colors [T, h, w, q] normalised with the orientation applied to
    component 0, flipped)."""
    T, h, w, _ = feature_map.shape
    rows = rows_of(feature_map, normalize)
    mean, cov, xc = moments(rows)
    V, evals = components(cov, q)
    norm = min_max(rows @ V.T).reshape(T, h, w, q)
    flip = border_flip(norm[..., 0]) if orient == "border" else False
    flip ^= bool(invert)
    if flip:
        norm[..., 0] = 1.0 - norm[..., 0]
    return {"mean": mean, "cov": cov, "xc": xc, "evals": evals, "V": V, "colors": norm, "flipped": flip}


def nearest_indices(n_src: int, n_dst: int) -> np.ndarray:
    """F.interpolate(mode="nearest"): destination index y reads source index floor(y n_src / n_dst)."""
    return (np.arange(n_dst, dtype=np.int64) * n_src) // n_dst


def upsample(tok: np.ndarray, H: int, W: int) -> np.ndarray:
    """tok [T, h, w] -> [T, H, W]."""
    return tok[:, nearest_indices(tok.shape[1], H)][:, :, nearest_indices(tok.shape[2], W)]


# ---- checks ---------------------------------------------------------------------------------------------------------------
def check_moments(got_cov: np.ndarray, ref_cov: np.ndarray, bound: np.ndarray, what: str = "cov") -> float:
    """Asserts the per-element bound; returns the worst error / bound ratio."""
    err = np.abs(got_cov.astype(np.float64) - ref_cov)
    ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print(f"{what}: max |err| {err.max():.3e}, worst err / bound {ratio:.3e}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements beyond the bound, worst ratio {ratio:.3f}"
    return ratio


def match_colors(got_c0: np.ndarray, gold_c0: np.ndarray, tol: float, what: str = "colors") -> int:
    """got / gold: normalised component 0, any shape.  +1 when got == gold within tol, -1 when got == 1 - gold."""
    got, gold = got_c0.astype(np.float64).ravel(), gold_c0.astype(np.float64).ravel()
    same, mirror = np.abs(got - gold).max(), np.abs(got - (1.0 - gold)).max()
    print(f"{what}: max |got - gold| {same:.3e}, max |got - (1 - gold)| {mirror:.3e}, tol {tol:.3e}")
    assert min(same, mirror) <= tol, f"{what}: {min(same, mirror):.3e} > {tol:.3e}"
    return 1 if same <= mirror else -1


def check_mask(got_tok: np.ndarray, want_tok: np.ndarray, c0: np.ndarray, thr: float, tol: float, max_excluded: int = 2,
               what: str = "mask") -> int:
    """Token masks (bool / 0-255, any shape) equal except where the float64 normalised colour `c0` of the thresholded sign is
    within tol of thr; at most max_excluded such tokens.  Returns how many were excluded."""
    near = np.abs(c0.astype(np.float64).ravel() - thr) <= tol
    assert near.sum() <= max_excluded, f"{what}: {int(near.sum())} tokens within {tol:.1e} of {thr}"
    diff = (got_tok.ravel() > 0) != (want_tok.ravel() > 0)
    bad = int((diff & ~near).sum())
    print(f"{what} @ {thr}: {int(diff.sum())} differing tokens, {int(near.sum())} near the threshold")
    assert bad == 0, f"{what} @ {thr}: {bad} tokens differ away from the threshold"
    return int(near.sum())
