"""Baseline JPEG DECODING (SOF0, 8 bit, 4:2:0, one interleaved scan, any Huffman tables, any restart interval) restated in numpy and
plain Python from docs/JPEG_DECODE.md: the arithmetic the device decoder (csrc/jpeg_decode.hip, csrc/jpeg_entropy.h) is held to, bit
for bit.  Written from the document, not from the kernels: the entropy decoder walks one Python integer window over the unstuffed
bytes with a full 16-bit code table, the inverse DCT transforms every block at once as int32 arrays (numpy wraps them, as the
document demands), the upsampling works on whole planes.  Nothing here imports the package under test.

    parse(data)                          the fields of the header this restatement needs (asserts the eligible form)
    coefficients(data)                   int16 [MCUs, 6, 64], zigzag order (blocks Y00 Y01 Y10 Y11 Cb Cr)
    pixels(coef, qtables, H, W)          uint8 [H, W, 3];  qtables int [3, 64] zigzag, one per component
    decode(data)                         the whole file -> uint8 [H, W, 3]

`faults` plants one deviation by name (FAULTS); tests/test_jpeg_decode_reference.py shows that the comparison with Pillow (or with
the encoder's coefficients) notices each.  `exact=True` (the default of `pixels`) asserts that no 32-bit operation wrapped: true for
every file an encoder made from 8-bit samples (docs/JPEG_DECODE.md section 2)."""
import numpy as np

from jpeg_ref import ZIGZAG

FAULTS = ("bias_swapped", "padded_context", "row_shift_17", "colour_constant", "extend_off_by_one", "zrl_15", "dc_no_reset",
          "stuffing_kept")


# ---- the header ----------------------------------------------------------------------------------------------------------------
def parse(data):
    """dict(H, W, qt int [3, 64] zigzag, huff [(dc (bits, vals), ac (bits, vals))] * 3, R, scan bytes without EOI)"""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    i, dqt, dht, R, sof = 2, {}, {}, 0, None
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
        if marker == 0xC0:
            assert seg[0] == 8 and seg[5] == 3
            sof = seg
        assert marker not in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF), "not baseline"
        if marker == 0xDA:
            break
    H, W = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big")
    comps = [tuple(sof[6 + 3 * c:9 + 3 * c]) for c in range(3)]
    assert [c[:2] for c in comps] == [(1, 0x22), (2, 0x11), (3, 0x11)], comps
    assert seg[0] == 3 and tuple(seg[7:10]) == (0, 63, 0), "one interleaved scan of everything"
    huff = []
    for c in range(3):
        assert seg[1 + 2 * c] == c + 1
        td, ta = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
        huff.append((dht[td], dht[0x10 | ta]))
    end = len(data) - 2 if data[-2:] == b"\xff\xd9" else len(data)
    return dict(H=H, W=W, qt=np.stack([dqt[c[2]] for c in comps]), huff=huff, R=R, scan=data[i:end])


# ---- entropy decoding (T.81 F.2.2) ---------------------------------------------------------------------------------------------
def _code_lookup(bits, vals):
    """for every 16-bit window: (code length, symbol), length 0 where no code matches -- the canonical codes of T.81 Annex C"""
    length = np.zeros(1 << 16, dtype=np.int64)
    symbol = np.zeros(1 << 16, dtype=np.int64)
    code, k = 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            lo = code << (16 - n)
            length[lo:lo + (1 << (16 - n))] = n
            symbol[lo:lo + (1 << (16 - n))] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return length.tolist(), symbol.tolist()


class _Bits:
    """MSB-first reader over one restart interval's bytes; beyond the end the bits are zero"""

    def __init__(self, raw, faults):
        if "stuffing_kept" not in faults:
            raw = raw.replace(b"\xff\x00", b"\xff")
        self.n = 8 * len(raw)
        self.buf = raw + bytes(8)
        self.pos = 0

    def window(self):   # the next 32 bits
        if self.pos >= self.n:
            return 0
        b = self.pos >> 3
        return ((int.from_bytes(self.buf[b:b + 5], "big") << (self.pos & 7)) >> 8) & 0xFFFFFFFF


def _extend(v, s, faults):
    if s == 0 or v >> (s - 1):
        return v
    return v - (1 << s) + (0 if "extend_off_by_one" in faults else 1)


def coefficients(data, faults=(), info=None):
    """int16 [MCUs, 6, 64] in zigzag order.  `info` (a dict) receives overrun / leftover observations of a damaged stream."""
    p = parse(data)
    mcus = -(-p["H"] // 16) * -(-p["W"] // 16)
    tables = [(_code_lookup(*dc), _code_lookup(*ac)) for dc, ac in p["huff"]]
    scan = p["scan"]
    # the intervals: split at FF D0 .. FF D7
    raw = np.frombuffer(scan, dtype=np.uint8)
    at = np.flatnonzero((raw[:-1] == 0xFF) & (raw[1:] >= 0xD0) & (raw[1:] <= 0xD7)) if len(raw) > 1 else np.zeros(0, dtype=np.int64)
    starts, ends = [0] + [int(a) + 2 for a in at], [int(a) for a in at] + [len(scan)]
    R = p["R"] if p["R"] else mcus
    assert len(starts) == -(-mcus // R), (len(starts), mcus, R)
    out = np.zeros((mcus, 6, 64), dtype=np.int64)
    pred = [0, 0, 0]
    bad = False
    for it, (a, b) in enumerate(zip(starts, ends)):
        bits = _Bits(scan[a:b], faults)
        if "dc_no_reset" not in faults:
            pred = [0, 0, 0]
        for m in range(it * R, min(mcus, (it + 1) * R)):
            for blk in range(6):
                comp = max(0, blk - 3)
                (dl, ds), (al, as_) = tables[comp]
                w = bits.window()
                n, s = dl[w >> 16], ds[w >> 16]
                assert n, "no DC code matches"
                diff = _extend(((w << n) & 0xFFFFFFFF) >> (32 - s) if s else 0, s, faults)
                bits.pos += n + s
                pred[comp] += diff
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
                        k += 15 if "zrl_15" in faults else 16
                        continue
                    k += r
                    if k > 63:
                        bad = True
                        break
                    out[m, blk, k] = _extend(((w << n) & 0xFFFFFFFF) >> (32 - s), s, faults)
                    k += 1
        if bits.pos > bits.n or bits.n - bits.pos > 7:
            bad = True
    if info is not None:
        info["damaged"] = bad
    return out.astype(np.int16)


# ---- dequantisation and the inverse DCT ----------------------------------------------------------------------------------------
def _pass(i, n):
    """one 1-D pass over i[0 .. 7] (arrays of any integer type: the type decides whether the arithmetic wraps)"""
    def D(x):
        return (x + (1 << (n - 1))) >> n
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return [D(t10 + a3), D(t11 + a2), D(t12 + a1), D(t13 + a0), D(t13 - a0), D(t12 - a1), D(t11 - a2), D(t10 - a3)]


def _idct_typed(nat, dtype, row_shift):
    x = nat.astype(dtype)                                                         # [N, v, u]
    with np.errstate(over="ignore"):
        cols = np.stack(_pass([x[:, k, :] for k in range(8)], 11), axis=1)       # over v, for every column u
        rows = np.stack(_pass([cols[:, :, k] for k in range(8)], row_shift), axis=2)
    return rows


def idct(coef, q, faults=(), exact=True):
    """coef int [N, 64] zigzag, q int [64] zigzag -> samples uint8-valued int64 [N, 8, 8]"""
    nat = np.zeros((coef.shape[0], 64), dtype=np.int64)
    nat[:, ZIGZAG] = coef.astype(np.int64) * np.asarray(q, dtype=np.int64)
    nat = nat.reshape(-1, 8, 8)
    shift = 17 if "row_shift_17" in faults else 18
    got = _idct_typed(nat, np.int32, shift).astype(np.int64)
    if exact:
        assert np.array_equal(got, _idct_typed(nat, np.int64, shift)), "a 32-bit operation wrapped"
    return np.clip(got + 128, 0, 255)


# ---- upsampling and colour -----------------------------------------------------------------------------------------------------
def upsample(c, H, W, faults=(), padded=None):
    """h2v2 'fancy' upsampling of the REAL chroma plane c [ch, cw] -> [H, W]"""
    ch, cw = c.shape
    c = c.astype(np.int64)
    up = c[np.maximum(np.arange(ch) - 1, 0)]
    down = c[np.minimum(np.arange(ch) + 1, ch - 1)]
    if "padded_context" in faults and padded is not None and padded.shape[0] > ch:
        down = down.copy()
        down[-1] = padded[ch, :cw]
    s = np.empty((2 * ch, cw), dtype=np.int64)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + down
    left = s[:, np.maximum(np.arange(cw) - 1, 0)]
    right = s[:, np.minimum(np.arange(cw) + 1, cw - 1)]
    be, bo = (7, 8) if "bias_swapped" in faults else (8, 7)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + be) >> 4, (3 * s + right + bo) >> 4
    return out[:H, :W]


def pixels(coef, qt, H, W, faults=(), exact=True):
    mh, mw = -(-H // 16), -(-W // 16)
    coef = np.asarray(coef).astype(np.int64).reshape(mh, mw, 6, 64)
    y = np.zeros((16 * mh, 16 * mw), dtype=np.int64)
    for k, (by, bx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        blk = idct(coef[:, :, k].reshape(-1, 64), qt[0], faults, exact).reshape(mh, mw, 8, 8)
        y.reshape(mh, 16, mw, 16)[:, 8 * by:8 * by + 8, :, 8 * bx:8 * bx + 8] = blk.transpose(0, 2, 1, 3)
    planes = []
    for c in (1, 2):
        blk = idct(coef[:, :, 3 + c].reshape(-1, 64), qt[c], faults, exact).reshape(mh, mw, 8, 8)
        full = blk.transpose(0, 2, 1, 3).reshape(8 * mh, 8 * mw)
        planes.append(upsample(full[:-(-H // 2), :-(-W // 2)], H, W, faults, padded=full) - 128)
    y, (cb, cr) = y[:H, :W], planes
    # (of the off-by-one constants only a few can be seen at all on -128 .. 127; 116129 shows at cb = +-125)
    k_b = 116129 if "colour_constant" in faults else 116130
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((k_b * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data, faults=(), exact=True):
    p = parse(data)
    return pixels(coefficients(data, faults), p["qt"], p["H"], p["W"], faults, exact)
