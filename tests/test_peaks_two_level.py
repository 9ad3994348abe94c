"""corr_peaks_kernel's two-level candidate selection (csrc/track_mfma.hip, `peaks_group_op`), restated in NumPy.

The kernel holds, per lane half, the 16 same-parity cells of every 32-cell step as one GROUP of accumulator registers.
Level 1 tags each raw float with its register index in the low 4 mantissa bits and keeps the group's sorted top-3 as signed
integers; level 2 turns the group's top-2 into fixed-point keys ((int)x << 13 | step << 4 | register) and inserts them into
the lane half's six-entry list; the group's third value feeds a running maximum `third`.  The record epilogue escalates a
source to the exact tier when a sixth list entry OR the key-domain bound of `third` reaches the band.

The argument (restated from the kernel comment):
  * the accumulator is 2^17 rho < 2^20, so the four tag bits are fraction bits: (int)tagged == (int)x, the keys level 2
    builds are the keys the one-level program built;
  * level 1 orders by (float bits >> 4, register), which refines the order of (int)x; it can misorder only values of EQUAL
    integer part, and it drops all but two values of a group.  Every dropped value's key is <= K3 = (int)third << 13 | 0x1fff;
  * K3 < thr: no dropped key reaches the band, so the true maximum was inserted and the list holds the keys >= thr exactly
    as the one-level program's list does: the record is IDENTICAL.  K3 >= thr: the source is flagged (ncand = KC + 1).
  * the band itself (EPS_PK against the fp16 operand roundings: test_numeric_claims.py) is untouched: the tag's 2^-19
    relative perturbation never reaches a key.

Checked for every source below: (a) the first-index arg-max of the exact fp32 map is a candidate or the source is flagged,
for kernel-side maps within the proven 2^-10 of the exact one; (b) an unflagged record equals the one-level program's.
"""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = open(os.path.join(HERE, "..", "dino_tracker_amd", "csrc", "track_mfma.hip")).read()
EPS_PK = float(re.search(r"constexpr float EPS_PK = ([0-9.eE+-]+)f;", SRC).group(1))
VAL_BITS = int(re.search(r"constexpr int PK_VAL_BITS = (\d+);", SRC).group(1))
IDX_BITS = int(re.search(r"constexpr int PK_IDX_BITS = (\d+);", SRC).group(1))
TOP = int(re.search(r"constexpr int PK_TOP = (\d+);", SRC).group(1))
KC = int(re.search(r"constexpr int KC = (\d+);", SRC).group(1))
CN = 32                       # pw_pad: map rows are padded to whole 32-cell steps
BAND = int(np.float32(EPS_PK) * np.float32(1 << VAL_BITS)) << IDX_BITS
ERR16 = 2.0 ** -10            # |rho16 - rho|: the operand-rounding bound test_numeric_claims.py proves


def _pw_pad(pw):
    return (pw + CN - 1) // CN * CN


def _groups(acc, pw):
    """acc: fp32 [ph, pw_pad] accumulator map (2^17 rho16, pad columns 0).  Yields (step, lane half, values[16]) with the
    kernel's checkerboard: register r of half h holds cell 32 st + 8 (r >> 2) + 2 (r & 3) + (h ^ (map row & 1))."""
    flat = acc.reshape(-1)
    tiles_per_row = _pw_pad(pw) // 32
    r = np.arange(16)
    for st in range(flat.size // 32):
        odd = (st // tiles_per_row) & 1
        for h in range(2):
            yield st, h, flat[32 * st + 8 * (r >> 2) + 2 * (r & 3) + (h ^ odd)]


def _key(x, st, r):
    # v_cvt_i32_f32 truncates towards zero; the shift of a negative integer is arithmetic
    return (int(np.trunc(np.float32(x))) << IDX_BITS) | (st << 4) | int(r)


def _top(values, n):
    """sorted insertion into n zero-initialised entries == the n largest of (values + n zeros)"""
    return sorted(list(values) + [0] * n, reverse=True)[:n]


def _lists_one_level(acc, pw):
    keys = [[], []]
    for st, h, x in _groups(acc, pw):
        keys[h] += [_key(x[r], st, r) for r in range(16)]
    return [_top(keys[0], TOP), _top(keys[1], TOP)], 0


def _lists_two_level(acc, pw):
    keys = [[], []]
    third = [0, 0]
    for st, h, x in _groups(acc, pw):
        tagged = (x.astype(np.float32).view(np.int32) & ~np.int32(15)) | np.arange(16, dtype=np.int32)   # v_and_or_b32
        g = _top([int(t) for t in tagged], 3)
        for gx in g[:2]:
            val = np.array([gx], dtype=np.int32).view(np.float32)[0]
            keys[h].append(_key(val, st, gx & 15))
        third[h] = max(third[h], g[2])
    t = np.array([max(third)], dtype=np.int32).view(np.float32)[0]
    k3 = (int(np.trunc(t)) << IDX_BITS) | ((1 << IDX_BITS) - 1)
    return [_top(keys[0], TOP), _top(keys[1], TOP)], k3


def _record(lists, k3, pw, one_level):
    """the record epilogue: (candidate cells in list order, flagged for the exact tier)"""
    v, o = lists
    amax_i = max(v[0], o[0])
    thr = amax_i - BAND
    pwp = _pw_pad(pw)
    tiles_per_row = pwp // 32
    cand = []
    for k, xi in enumerate(v + o):
        if xi >= thr:
            tag = xi & ((1 << IDX_BITS) - 1)
            r, st = tag & 15, tag >> 4
            pc = st * 32 + 8 * (r >> 2) + 2 * (r & 3) + ((0 if k < TOP else 1) ^ ((st // tiles_per_row) & 1))
            row, col = divmod(pc, pwp)
            cand.append(row * pw + min(col, pw - 1))
    flagged = v[TOP - 1] >= thr or o[TOP - 1] >= thr or thr <= 0 or (not one_level and k3 >= thr) or len(cand) > KC
    return cand, flagged, amax_i >> IDX_BITS


def _padded(rho, pw):
    out = np.zeros((rho.shape[0], _pw_pad(pw)), dtype=np.float32)
    out[:, :pw] = rho
    return out


def _check(rho, rng, label):
    """rho: exact fp32 map [ph, pw].  The kernel sees 2^17 (rho + e), |e| <= 2^-10: once with e = 0, once random, once with
    the exact maximum pushed down and everything else up by the full bound."""
    ph, pw = rho.shape
    first = int(np.argmax(rho.reshape(-1)))   # first index among equal maxima
    errs = [np.zeros_like(rho), rng.uniform(-ERR16, ERR16, rho.shape).astype(np.float32), np.full_like(rho, ERR16)]
    errs[2].reshape(-1)[first] = -ERR16
    flagged_any = False
    for e in errs:
        acc = _padded(((rho.astype(np.float64) + e) * 2.0 ** VAL_BITS).astype(np.float32), pw)
        cand2, flag2, amax2 = _record(*_lists_two_level(acc, pw), pw, False)
        cand1, flag1, amax1 = _record(*_lists_one_level(acc, pw), pw, True)
        assert flag2 or first in cand2, (label, first, cand2)
        assert flag2 or (cand2 == cand1 and flag1 == flag2 and amax1 == amax2), (label, cand1, cand2)
        assert flag2 or not flag1, label   # the two-level program never clears a flag the one-level program raises
        flagged_any |= flag2
    return flagged_any


def _peaked(rng, ph, pw, n_peaks, height=0.8):
    """a smooth-ish map: low noise plus a few Gaussian bumps (what a correlation map of video features looks like)"""
    yy, xx = np.mgrid[0:ph, 0:pw]
    m = rng.normal(0.05, 0.05, (ph, pw))
    for _ in range(n_peaks):
        cy, cx, s = rng.uniform(0, ph), rng.uniform(0, pw), rng.uniform(0.7, 3.0)
        m += height * rng.uniform(0.6, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return np.clip(m, -1, 1).astype(np.float32)


def test_seeded_maps_argmax_is_candidate_or_flagged():
    rng = np.random.default_rng(7)
    for trial in range(24):
        ph, pw = [(9, 37), (12, 64), (7, 121), (16, 33)][trial % 4]
        _check(_peaked(rng, ph, pw, 1 + trial % 5), rng, ("peaked", trial))
    for trial in range(8):   # white noise: many near-maximal cells far apart
        _check(rng.uniform(-1, 1, (8, 70)).astype(np.float32), rng, ("noise", trial))
    for trial in range(8):   # broad plateaus: most cells inside the band
        _check((0.5 + 1e-4 * rng.standard_normal((6, 45))).astype(np.float32), rng, ("flat", trial))


def test_exact_ties():
    rng = np.random.default_rng(8)
    for trial in range(12):
        m = _peaked(rng, 10, 50, 2)
        top = float(m.max()) + 0.01
        cells = rng.choice(m.size, size=2 + trial % 4, replace=False)
        m.reshape(-1)[cells] = top               # equal maxima anywhere in the map
        _check(m, rng, ("ties", trial))
    m = np.full((6, 40), 0.25, dtype=np.float32)  # every cell ties
    assert _check(m, rng, "all equal")


def test_plateau_of_three_equal_maxima_inside_one_group():
    """three (and more) equal maxima in the same-parity cells of one 16-cell segment: level 1 keeps two, the third
    reaches `third` with the maximum's integer part -> flagged, whatever the register order"""
    rng = np.random.default_rng(9)
    for row in (2, 3):            # even and odd map rows (the lane halves swap)
        for n in (3, 4, 8):
            m = (0.1 * rng.random((6, 64))).astype(np.float32)
            cols = 32 + 2 * rng.choice(16, size=n, replace=False)   # same parity, one step
            m[row, cols] = 0.75
            assert _check(m, rng, ("plateau", row, n))
            # first index = the lowest register: exactly the one a (bits, register) order ranks last among equals
            assert int(np.argmax(m.reshape(-1))) == row * 64 + int(cols.min())


def test_two_band_members_in_one_group_and_a_third_in_the_other_half():
    """two band members in one group and one in the other lane half are all inserted: identical to the one-level record,
    and not flagged (the group's third value is far below the band)"""
    rng = np.random.default_rng(10)
    for row in (1, 4):
        m = (0.1 * rng.random((6, 64))).astype(np.float32)
        m[row, 34] = 0.7500        # exact maximum
        m[row, 40] = 0.7495        # same parity, same step: same group
        m[row, 37] = 0.7490        # other parity: the other lane half
        assert not _check(m, rng, ("two plus one", row))
    # a third member of the SAME group inside the band flags the source
    m = (0.1 * rng.random((6, 64))).astype(np.float32)
    m[2, 34], m[2, 40], m[2, 44] = 0.7500, 0.7495, 0.7490
    assert _check(m, rng, "three in a group")


def test_zero_and_negative_maps_are_flagged():
    rng = np.random.default_rng(11)
    assert _check(np.zeros((5, 40), dtype=np.float32), rng, "zeros")
    assert _check(np.full((5, 40), -0.3, dtype=np.float32), rng, "negative constant")
    assert _check((-0.5 * rng.random((5, 40)) - 0.01).astype(np.float32), rng, "negative random")
    m = (-0.5 * rng.random((5, 40)) - 0.01).astype(np.float32)
    m[3, 17] = 0.6                 # one positive cell among negatives: found, not flagged
    assert not _check(m, rng, "one positive")


def test_tag_bits_are_fraction_bits():
    """(int)tagged == (int)x for every accumulator value the kernel can see (|x| <= 2^17 (1 + band) < 2^20), and the tagged
    order refines the order of the integer parts"""
    rng = np.random.default_rng(12)
    x = np.concatenate([rng.uniform(0, 2.0 ** VAL_BITS * 1.01, 20000), rng.uniform(0, 4, 2000),
                        np.arange(0, 2.0 ** VAL_BITS, 977.0)]).astype(np.float32)
    for r in (0, 7, 15):
        t = ((x.view(np.int32) & ~np.int32(15)) | np.int32(r)).view(np.float32)
        assert (np.trunc(t) == np.trunc(x)).all()
        assert (np.abs(t - x) <= np.maximum(np.abs(x) * 2.0 ** -19, 2.0 ** -145)).all()   # (x = 0: the tag alone, a denormal)
    order = np.argsort(x.view(np.int32) >> 4, kind="stable")
    assert (np.diff(np.trunc(x[order])) >= 0).all()
