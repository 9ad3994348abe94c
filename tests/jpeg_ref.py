"""Baseline JPEG (SOF0, 8 bit, 4:2:0, interleaved scan, restart intervals) restated in numpy from docs/JPEG.md: the arithmetic the
device encoder (csrc/jpeg.hip) is held to, byte for byte.  Written from the document, not from the kernels: whole planes are
padded and downsampled, every block is transformed at once as an array, and the entropy coder builds one big integer per
restart interval.  Nothing here imports the package under test.

    coefficients(img, quality)      int16 [MCUs, 6, 64], zigzag order (blocks Y00 Y01 Y10 Y11 Cb Cr)
    scan(coef, R)                   the entropy-coded segment: intervals, RST markers, final padding (no EOI)
    header(h, w, quality, R)        SOI .. SOS
    encode(img, quality, R)         the whole file

`faults` plants one deviation by name (FAULTS); tests/test_jpeg_reference.py shows that the comparison with Pillow notices each."""
import numpy as np

RESTART = 16   # the library's restart interval in MCUs (docs/JPEG.md)

FAULTS = ("chroma_rows_before_downsample", "transformed_padding", "bias_from_2", "quant_floor", "rst_no_wrap", "dc_no_reset",
          "pad_zero", "missing_stuffing", "missing_zrl", "eob_always")

# natural (row-major) index of the k-th zigzag coefficient
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

# Annex K.1: the two base quantisation tables, natural order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def _ac_values(head, rows):
    """the tail of both Annex K AC value lists: for every run nibble the sizes lo .. 0xA"""
    return head + [(r << 4) | s for r, lo in rows for s in range(lo, 0xB)]


# Annex K.3: (counts of codes of length 1 .. 16, values in code order) of the four typical tables
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], _ac_values(
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82],
    [(0, 9), (1, 6), (2, 5), (3, 4), (4, 3), (5, 3), (6, 3), (7, 3), (8, 3), (9, 2), (10, 2), (11, 2), (12, 2), (13, 2), (14, 1),
     (15, 1)]))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], _ac_values(
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
     0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A],
    [(3, 5), (4, 3), (5, 3), (6, 3), (7, 3), (8, 2), (9, 2), (10, 2), (11, 2), (12, 2), (13, 2), (14, 2), (15, 2)]))


def quant_tables(quality):
    """(luma, chroma) int arrays of 64 in ZIGZAG order, as a DQT segment stores them."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality must be 1 .. 100, got {quality}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255)[ZIGZAG] for base in (BASE_LUMA, BASE_CHROMA))


def code_table(bits, vals):
    """symbol -> (code, length): canonical codes, shortest first, in the order of `vals`"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return table


# ---- colour, edges, downsampling -----------------------------------------------------------------------------------------------
def planes(img, faults=()):
    """uint8 [H, W, 3] -> (Y [16 mh, 16 mw], Cb, Cr [8 mh, 8 mw]) as int64, padded to whole MCUs by the edge rules"""
    H, W = img.shape[:2]
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    mh, mw = -(-H // 16), -(-W // 16)

    def grow(p, rows, cols):
        return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")

    def down(p):
        rows = 16 * mh if "chroma_rows_before_downsample" in faults else H + (H & 1)
        p = grow(p, rows, 16 * mw)                      # columns to the MCU boundary, rows only to an even count
        s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        first = 2 if "bias_from_2" in faults else 1
        bias = (np.arange(s.shape[1]) + (first - 1)) % 2 + 1   # 1, 2, 1, 2, ...
        return grow((s + bias) >> 2, 8 * mh, 8 * mw)    # then the last downsampled row to the MCU boundary
    return grow(y, 16 * mh, 16 * mw), down(cb), down(cr)


# ---- forward DCT ---------------------------------------------------------------------------------------------------------------
def _pass(d, first):
    """one 1-D pass over d[0 .. 7] (arrays); constants are round(c * 8192)"""
    def descale(x, n):
        return (x + (1 << (n - 1))) >> n
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = descale(z1 + t13 * 6270, n)
    o[6] = descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7] = descale(t4 + z1 + z3, n)
    o[5] = descale(t5 + z2 + z4, n)
    o[3] = descale(t6 + z2 + z3, n)
    o[1] = descale(t7 + z1 + z4, n)
    return o


def fdct(blocks):
    """int64 [N, 8, 8] level-shifted samples -> [N, 8, 8] = 8 x DCT, rows first"""
    rows = np.stack(_pass([blocks[:, :, k] for k in range(8)], True), axis=2)      # [N, y, u]
    return np.stack(_pass([rows[:, k, :] for k in range(8)], False), axis=1)       # [N, v, u]


def quantise(c, qzz, faults=()):
    """[N, 8, 8] -> [N, 64] zigzag; round half away from zero, truncating divisions"""
    q8 = 8 * np.asarray(qzz, dtype=np.int64)
    z = c.reshape(-1, 64)[:, ZIGZAG]
    pos = (np.abs(z) + q8 // 2) // q8
    if "quant_floor" in faults:
        return np.where(z < 0, (z + q8 // 2) // q8, pos)
    return np.where(z < 0, -pos, pos)


def coefficients(img, quality, faults=()):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    H, W = img.shape[:2]
    ql, qc = quant_tables(quality)
    y, cb, cr = planes(img, faults)
    mh, mw = y.shape[0] // 16, y.shape[1] // 16

    def blocks(p):   # [rows, cols] -> [rows / 8, cols / 8, 8, 8]
        return p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)
    yq = quantise(fdct(blocks(y).reshape(-1, 8, 8) - 128), ql, faults).reshape(2 * mh, 2 * mw, 64)
    out = np.zeros((mh, mw, 6, 64), dtype=np.int64)
    for k, (by, bx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, :, k] = yq[by::2, bx::2]
        if "transformed_padding" not in faults and k:
            dummy = ((2 * np.arange(mh) + by) >= -(-H // 8))[:, None] | ((2 * np.arange(mw) + bx) >= -(-W // 8))[None, :]
            out[:, :, k][dummy] = 0
            out[:, :, k, 0] = np.where(dummy, out[:, :, k - 1, 0], out[:, :, k, 0])
    out[:, :, 4] = quantise(fdct(blocks(cb).reshape(-1, 8, 8) - 128), qc, faults).reshape(mh, mw, 64)
    out[:, :, 5] = quantise(fdct(blocks(cr).reshape(-1, 8, 8) - 128), qc, faults).reshape(mh, mw, 64)
    assert np.abs(out[..., 1:]).max(initial=0) <= 1023 and np.abs(out[..., 0]).max() <= 1024
    return out.reshape(mh * mw, 6, 64).astype(np.int16)


# ---- entropy coding ------------------------------------------------------------------------------------------------------------
_TABLES = None


def _tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = tuple(code_table(*t) for t in (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA))
    return _TABLES


def _value_bits(v, size):
    return (v if v >= 0 else v - 1) & ((1 << size) - 1)


def _block_bits(z, diff, dc, ac, faults):
    """(bits, count) of one block as an integer, most significant bit first"""
    size = abs(diff).bit_length()
    acc, n = dc[size]
    acc, n = (acc << size) | _value_bits(diff, size), n + size
    last = 0
    for k in np.flatnonzero(z[1:]) + 1:
        run, v = int(k) - last - 1, int(z[k])
        if "missing_zrl" in faults:
            run &= 15
        while run > 15:
            code, length = ac[0xF0]
            acc, n, run = (acc << length) | code, n + length, run - 16
        size = abs(v).bit_length()
        code, length = ac[(run << 4) | size]
        acc, n = (((acc << length) | code) << size) | _value_bits(v, size), n + length + size
        last = int(k)
    if last < 63 or "eob_always" in faults:
        code, length = ac[0x00]
        acc, n = (acc << length) | code, n + length
    return acc, n


def scan(coef, R=RESTART, faults=()):
    dcl, acl, dcc, acc_c = _tables()
    coef = np.asarray(coef).astype(np.int64)
    out = bytearray()
    pred = [0, 0, 0]
    dropped = False
    for start in range(0, len(coef), R):
        if start:
            n = start // R - 1
            out += bytes([0xFF, 0xD0 + (n % 48 if "rst_no_wrap" in faults else n % 8)])
        if "dc_no_reset" not in faults:
            pred = [0, 0, 0]
        acc, nbits = 0, 0
        for mcu in coef[start:start + R]:
            for b in range(6):
                comp = max(0, b - 3)
                dc, ac = (dcl, acl) if comp == 0 else (dcc, acc_c)
                bits, n = _block_bits(mcu[b], int(mcu[b][0]) - pred[comp], dc, ac, faults)
                pred[comp] = int(mcu[b][0])
                acc, nbits = (acc << n) | bits, nbits + n
        pad = -nbits % 8
        acc, nbits = (acc << pad) | (0 if "pad_zero" in faults else (1 << pad) - 1), nbits + pad
        data = acc.to_bytes(nbits // 8, "big")
        if "missing_stuffing" in faults and not dropped and b"\xff" in data:
            i = data.index(b"\xff") + 1
            data, dropped = data[:i] + data[i:].replace(b"\xff", b"\xff\x00"), True
        else:
            data = data.replace(b"\xff", b"\xff\x00")
        out += data
    return bytes(out)


# ---- the file ------------------------------------------------------------------------------------------------------------------
def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(h, w, quality, R=RESTART):
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += _segment(0xDB, bytes([0]) + bytes(ql.astype(np.uint8))) + _segment(0xDB, bytes([1]) + bytes(qc.astype(np.uint8)))
    out += _segment(0xC0, bytes([8]) + int(h).to_bytes(2, "big") + int(w).to_bytes(2, "big") +
                    bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for ident, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, int(R).to_bytes(2, "big"))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(img, quality=90, R=RESTART, faults=()):
    img = np.asarray(img)
    return header(img.shape[0], img.shape[1], quality, R) + scan(coefficients(img, quality, faults), R, faults) + b"\xff\xd9"


# ---- helpers for the tests: reading a JPEG file's segments ------------------------------------------------------------------------
def split(data):
    """a JPEG file -> ([(marker, payload), ...] up to and including SOS, the entropy-coded bytes without EOI)"""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9", "not SOI .. EOI"
    i, segs = 2, []
    while True:
        assert data[i] == 0xFF, f"no marker at {i}"
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        segs.append((marker, bytes(data[i + 4:i + 2 + length])))
        i += 2 + length
        if marker == 0xDA:
            return segs, bytes(data[i:-2])


def tables_of(data):
    """(dict table id -> 64 DQT bytes, dict DHT id -> (bits, vals)) of a JPEG file, however its segments group them"""
    dqt, dht = {}, {}
    for marker, seg in split(data)[0]:
        k = 0
        while marker == 0xDB and k < len(seg):
            assert seg[k] >> 4 == 0, "16-bit quantisation table"
            dqt[seg[k] & 15] = list(seg[k + 1:k + 65])
            k += 65
        while marker == 0xC4 and k < len(seg):
            bits = list(seg[k + 1:k + 17])
            dht[seg[k]] = (bits, list(seg[k + 17:k + 17 + sum(bits)]))
            k += 17 + sum(bits)
    return dqt, dht


# ---- test pictures -------------------------------------------------------------------------------------------------------------
def picture(kind, h, w, seed=0):
    rng = np.random.default_rng(seed + 1000 * h + w)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(3 * x + y) % 256, (x + 2 * y) % 256, (255 - x - y) % 256], axis=-1).astype(np.uint8)
    if kind == "checker":      # 8 x 8 squares of black and white: flat blocks, DC differences of category 11
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((y // 8 + x // 8) % 2) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    if kind == "pm1":          # +-1 around 128: at a low quality everything quantises to zero
        return (128 + rng.integers(-1, 2, (h, w, 3))).astype(np.uint8)
    raise ValueError(kind)
