"""Writes tests/golden/fg_mask.npz by running the UN-MODIFIED reference preprocessing/create_fg_mask.py
`get_fg_mask_from_pca` on CPU (needs a reference checkout, see oracle/ref_harness.py):
    python tests/golden/make_golden_fgmask.py

Inputs come from tests/golden/fg_mask_data.py (seeded, bit-identical everywhere; their digests are stored).  Every call runs
under torch.manual_seed(0) (torch.pca_lowrank draws a random test matrix).  The function returns only the mask, so the
projection matrix is recorded by wrapping torch.pca_lowrank for the duration of the call, and the colours are formed from it as
the function forms them (fp32).

Stored per case X: X_colors0 (the reference's min-max normalised component 0, fp32 [T, h, w]), X_tok04 / X_tok06 (its token
masks at the two thresholds: the function called with img_size = the token grid), X_up04 (its mask at IMG_SIZE, threshold 0.4),
X_sign (+1 / -1: the reference's component against the float64 oracle with the raw sign rule), X_ref_dev (the reference's
largest deviation from the oracle's colours), X_ratio (lambda_2 / lambda_1), X_digest.

Asserted here, so that the tests can rely on it: lambda_2 / lambda_1 < 0.1, and no token's float64 colour within 1e-4 of a
threshold or its mirror image.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_harness  # noqa: E402
import fg_mask_data as D  # noqa: E402
import fg_mask_ref as R  # noqa: E402

OUT = os.path.join(HERE, "fg_mask.npz")
BAND = 1e-4


def main():
    ref_harness.load()
    import preprocessing.create_fg_mask as FG

    out = {}
    for case in D.CASES:
        T, C, h, w = D.CASES[case]
        feats = D.features(case)
        out[f"{case}_digest"] = np.array(D.digest(feats))
        fm = torch.from_numpy(feats).permute(0, 2, 3, 1).contiguous()      # [T, h, w, C], as create_fg_mask.run passes it

        recorded = []
        real = torch.pca_lowrank

        def recording(*a, **k):
            r = real(*a, **k)
            recorded.append(r[2].clone())
            return r

        def call(img_size, thr):
            torch.manual_seed(0)
            torch.pca_lowrank = recording
            try:
                return FG.get_fg_mask_from_pca(fm, img_size, q=3, interpolation="nearest", fg_mask_threshold=thr)
            finally:
                torch.pca_lowrank = real

        tok = {thr: call((h, w), thr) for thr in D.THRESHOLDS}
        up = call(D.IMG_SIZE[case], D.THRESHOLDS[0])
        assert all(torch.equal(recorded[0], v) for v in recorded[1:])       # the seed makes the calls repeat
        rows = torch.nn.functional.normalize(fm, dim=-1).reshape(-1, C)
        colors = rows @ recorded[0]
        mn, mx = colors.min(dim=0).values, colors.max(dim=0).values
        c0 = ((colors - mn) / (mx - mn))[:, 0].reshape(T, h, w).numpy()
        for thr in D.THRESHOLDS:                                           # the colours above are the function's own
            np.testing.assert_array_equal(tok[thr] > 0, c0 < np.float32(thr))

        orc = R.exact_pca(fm.numpy(), q=3)
        ratio = float(orc["evals"][1] / orc["evals"][0])
        assert ratio < 0.1, (case, ratio)
        o0 = orc["colors"][..., 0]
        same, mirror = np.abs(c0 - o0).max(), np.abs(c0 - (1.0 - o0)).max()
        sign = 1 if same <= mirror else -1
        ref_dev = float(min(same, mirror))
        for thr in (0.4, 0.6):
            assert (np.abs(o0 - thr) > BAND).all(), (case, thr, int((np.abs(o0 - thr) <= BAND).sum()))
        out[f"{case}_colors0"] = c0.astype(np.float32)
        out[f"{case}_tok04"] = (tok[0.4] > 0)
        out[f"{case}_tok06"] = (tok[0.6] > 0)
        out[f"{case}_up04"] = np.packbits(up > 0)
        out[f"{case}_sign"] = np.array(sign, dtype=np.int32)
        out[f"{case}_ref_dev"] = np.array(ref_dev)
        out[f"{case}_ratio"] = np.array(ratio)
        print(f"case {case}: lambda2/lambda1 {ratio:.4f}, ref_dev {ref_dev:.3e}, sign {sign:+d}, reference fg fraction @0.4 "
              f"{(tok[0.4] > 0).mean():.3f}")

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT} ({size / 1024:.0f} KiB)")
    assert size < 1 << 20


if __name__ == "__main__":
    main()
