"""Baseline JPEG decoding for every sampling the device decodes -- 4:2:0, 4:2:2, 4:4:4 in one interleaved scan, and one gray
component -- restated in numpy and plain Python from docs/JPEG_DECODE.md (sections 0, 1, 3, 3a, 3b, 4): the MCU schedule, the plane
geometry and the upsampling rules.  The pieces that do not depend on the sampling (the canonical code table, the bit reader, the
sign extension, the inverse DCT) are tests/jpeg_dec_ref.py's, imported, not edited.  Nothing here imports the package under test.

    parse(data)                                   the header's fields: H, W, sampling, factors, qt [C, 64], huff, R, scan, adobe
    coefficients(data)                            int16 [MCUs, B, 64], zigzag order, blocks in scan order (B = 6, 4, 3, 1)
    pixels(coef, qt, H, W, sampling)              uint8 [H, W, 3], for GRAY uint8 [H, W]
    decode(data)                                  the whole file

`faults` plants one deviation by name (FAULTS); tests/test_jpeg_sampling_reference.py shows that the comparison with Pillow notices
each."""
import numpy as np

from jpeg_dec_ref import _Bits, _code_lookup, _extend, idct, upsample as _h2v2_fancy

S420, S422, S444, GRAY = 0, 1, 2, 3
NAMES = {S420: "4:2:0", S422: "4:2:2", S444: "4:4:4", GRAY: "gray"}
FACTORS = {(0x22, 0x11, 0x11): S420, (0x21, 0x11, 0x11): S422, (0x11, 0x11, 0x11): S444}
# per sampling: the luma blocks of an MCU in scan order as (block row, block column); then Cb and Cr follow (not for GRAY)
LUMA = {S420: ((0, 0), (0, 1), (1, 0), (1, 1)), S422: ((0, 0), (0, 1)), S444: ((0, 0),), GRAY: ((0, 0),)}
FAULTS = ("h2v1_bias_swapped", "h2v1_edge_filtered", "h2v1_narrow_filtered", "h2v2_narrow_filtered", "y1_before_y0",
          "gray_mcu_from_sof")


def blocks_per_mcu(sampling):
    return len(LUMA[sampling]) + (0 if sampling == GRAY else 2)


def mcu_size(sampling):
    """(height, width) of an MCU in pixels"""
    return 8 * (1 + max(b[0] for b in LUMA[sampling])), 8 * (1 + max(b[1] for b in LUMA[sampling]))


def mcu_grid(H, W, sampling):
    mh, mw = mcu_size(sampling)
    return -(-H // mh), -(-W // mw)


# ---- the header ----------------------------------------------------------------------------------------------------------------
def parse(data):
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    i, dqt, dht, R, sof, adobe = 2, {}, {}, 0, None, None
    while True:
        assert data[i] == 0xFF, f"no marker at {i}"
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        seg = data[i + 4:i + 2 + length]
        i += 2 + length
        k = 0
        while marker == 0xDB and k < len(seg):
            assert seg[k] >> 4 == 0, "16-bit quantisation table"
            dqt[seg[k] & 15] = np.array(list(seg[k + 1:k + 65]))
            k += 65
        while marker == 0xC4 and k < len(seg):
            bits = list(seg[k + 1:k + 17])
            dht[seg[k]] = (bits, list(seg[k + 17:k + 17 + sum(bits)]))
            k += 17 + sum(bits)
        if marker == 0xDD:
            R = int.from_bytes(seg[:2], "big")
        if marker == 0xEE and seg[:5] == b"Adobe":
            adobe = seg[11]
        if marker == 0xC0:
            assert seg[0] == 8 and seg[5] in (1, 3)
            sof = seg
        assert marker not in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF), "not baseline"
        if marker == 0xDA:
            break
    H, W, n = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big"), sof[5]
    comps = [tuple(sof[6 + 3 * c:9 + 3 * c]) for c in range(n)]
    assert [c[0] for c in comps] == [1, 2, 3][:n], comps
    factors = tuple(c[1] for c in comps)
    sampling = GRAY if n == 1 else FACTORS[factors]
    assert adobe is None or (n == 3 and adobe == 1), "an Adobe segment that does not say YCbCr"
    assert seg[0] == n and tuple(seg[1 + 2 * n:4 + 2 * n]) == (0, 63, 0), "one scan of everything"
    huff = []
    for c in range(n):
        assert seg[1 + 2 * c] == c + 1
        huff.append((dht[seg[2 + 2 * c] >> 4], dht[0x10 | (seg[2 + 2 * c] & 15)]))
    end = len(data) - 2 if data[-2:] == b"\xff\xd9" else len(data)
    return dict(H=H, W=W, sampling=sampling, factors=factors, qt=np.stack([dqt[c[2]] for c in comps]), huff=huff, R=R,
                scan=data[i:end], adobe=adobe)


# ---- entropy decoding: section 1 per block, the schedule of section 0 around it ----------------------------------------------------
def _schedule(p, faults):
    """(MCUs, the component of each block of an MCU)"""
    s = p["sampling"]
    if s == GRAY:
        if "gray_mcu_from_sof" in faults:     # as if the scan were interleaved: h x v blocks per MCU
            h, v = p["factors"][0] >> 4, p["factors"][0] & 15
            return -(-p["H"] // (8 * v)) * -(-p["W"] // (8 * h)), [0] * (h * v)
        return -(-p["H"] // 8) * -(-p["W"] // 8), [0]
    mh, mw = mcu_grid(p["H"], p["W"], s)
    return mh * mw, [0] * len(LUMA[s]) + [1, 2]


def coefficients(data, faults=(), info=None):
    """int16 [MCUs, B, 64] in zigzag order.  `info` (a dict) receives whether the stream was found damaged."""
    p = parse(data)
    mcus, comp_of = _schedule(p, faults)
    B = len(comp_of)
    tables = [(_code_lookup(*dc), _code_lookup(*ac)) for dc, ac in p["huff"]]
    scan = p["scan"]
    raw = np.frombuffer(scan, dtype=np.uint8)
    at = np.flatnonzero((raw[:-1] == 0xFF) & (raw[1:] >= 0xD0) & (raw[1:] <= 0xD7)) if len(raw) > 1 else np.zeros(0, dtype=np.int64)
    starts, ends = [0] + [int(a) + 2 for a in at], [int(a) for a in at] + [len(scan)]
    R = p["R"] if p["R"] else mcus
    assert len(starts) == -(-mcus // R), (len(starts), mcus, R)
    out = np.zeros((mcus, B, 64), dtype=np.int64)
    bad = False
    for it, (a, b) in enumerate(zip(starts, ends)):
        bits = _Bits(scan[a:b], ())
        pred = [0, 0, 0]
        for m in range(it * R, min(mcus, (it + 1) * R)):
            for blk in range(B):
                comp = comp_of[blk]
                (dl, ds), (al, as_) = tables[comp]
                w = bits.window()
                n, s = dl[w >> 16], ds[w >> 16]
                assert n, "no DC code matches"
                pred[comp] += _extend(((w << n) & 0xFFFFFFFF) >> (32 - s) if s else 0, s, ())
                bits.pos += n + s
                out[m, blk, 0] = pred[comp]
                k = 1
                while k < 64:
                    w = bits.window()
                    n, sym = al[w >> 16], as_[w >> 16]
                    assert n, "no AC code matches"
                    r, s = sym >> 4, sym & 15
                    bits.pos += n + s
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    if k > 63:
                        bad = True
                        break
                    out[m, blk, k] = _extend(((w << n) & 0xFFFFFFFF) >> (32 - s), s, ())
                    k += 1
        if bits.pos > bits.n or bits.n - bits.pos > 7:
            bad = True
    if info is not None:
        info["damaged"] = bad
    assert not (bad and faults), "the stream does not fit the schedule"
    return out.astype(np.int16)


# ---- planes, upsampling (sections 3, 3a, 3b), colour (section 4) ---------------------------------------------------------------------
def _plane(coef, q, rows, cols, exact):
    """blocks [rows * cols, 64] of one component, block row by block row -> samples [8 rows, 8 cols]"""
    blk = idct(coef.reshape(-1, 64), q, (), exact).reshape(rows, cols, 8, 8)
    return blk.transpose(0, 2, 1, 3).reshape(8 * rows, 8 * cols)


def h2v1(c, W, faults=()):
    """the REAL chroma plane c [H, cw] -> [H, W]: 'fancy' when cw > 2, each sample twice otherwise"""
    cw = c.shape[1]
    c = c.astype(np.int64)
    if cw <= 2 and "h2v1_narrow_filtered" not in faults:
        return np.repeat(c, 2, axis=1)[:, :W]
    li, ri = np.maximum(np.arange(cw) - 1, 0), np.minimum(np.arange(cw) + 1, cw - 1)   # the edges: 3 c + c = 4 c, the sample itself
    if "h2v1_edge_filtered" in faults and cw > 1:
        li[0], ri[-1] = 1, cw - 2
    be, bo = (2, 1) if "h2v1_bias_swapped" in faults else (1, 2)
    out = np.empty((c.shape[0], 2 * cw), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * c + c[:, li] + be) >> 2, (3 * c + c[:, ri] + bo) >> 2
    return out[:, :W]


def h2v2(c, H, W, faults=()):
    """the REAL chroma plane c [ch, cw] -> [H, W]: section 3's filter when cw > 2, each sample 2 x 2 otherwise"""
    if c.shape[1] <= 2 and "h2v2_narrow_filtered" not in faults:
        return np.repeat(np.repeat(c.astype(np.int64), 2, axis=0), 2, axis=1)[:H, :W]
    return _h2v2_fancy(c, H, W)


def pixels(coef, qt, H, W, sampling, faults=(), exact=True, gray_factors=0x11):
    luma = LUMA[sampling]
    if sampling == GRAY and "gray_mcu_from_sof" in faults:
        h, v = gray_factors >> 4, gray_factors & 15
        luma = tuple((by, bx) for by in range(v) for bx in range(h))
    if sampling == S422 and "y1_before_y0" in faults:
        luma = luma[::-1]
    bh, bw = 1 + max(b[0] for b in luma), 1 + max(b[1] for b in luma)
    mh, mw = -(-H // (8 * bh)), -(-W // (8 * bw))
    B = len(luma) + (0 if sampling == GRAY else 2)
    coef = np.asarray(coef).astype(np.int64).reshape(mh, mw, B, 64)
    y = np.zeros((8 * bh * mh, 8 * bw * mw), dtype=np.int64)
    for k, (by, bx) in enumerate(luma):
        blk = idct(coef[:, :, k].reshape(-1, 64), qt[0], (), exact).reshape(mh, mw, 8, 8)
        y.reshape(mh, 8 * bh, mw, 8 * bw)[:, 8 * by:8 * by + 8, :, 8 * bx:8 * bx + 8] = blk.transpose(0, 2, 1, 3)
    y = y[:H, :W]
    if sampling == GRAY:
        return y.astype(np.uint8)
    ch, cw = -(-H // bh), -(-W // bw)                       # the real chroma plane
    planes = []
    for c in (1, 2):
        real = _plane(coef[:, :, len(luma) + c - 1], qt[c], mh, mw, exact)[:ch, :cw]
        up = real if sampling == S444 else h2v1(real, W, faults) if sampling == S422 else h2v2(real, H, W, faults)
        planes.append(up - 128)
    cb, cr = planes
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data, faults=(), exact=True):
    p = parse(data)
    return pixels(coefficients(data, faults), p["qt"], p["H"], p["W"], p["sampling"], faults, exact, p["factors"][0])
