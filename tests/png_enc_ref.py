"""A plain-Python / numpy restatement of the two bit-defined stages of docs/PNG_ENCODE.md: the PNG row filters with the adaptive rule,
and the CRC-32 with its combination of pieces.  It is what the GPU tests compare the filter stage with byte for byte and what the CPU
tests hold against png_ref's unfilter, zlib.crc32 and Pillow; it shares no code with the library.  `FAULTS` plants single mistakes
that tests/test_png_encode_reference.py must notice."""
import struct
import zlib

import numpy as np

ADAPTIVE = 5
POLY = 0xEDB88320          # reflected: bit 31 is x^0

# planted faults (tests): a set of names
FAULTS = set()


# ---- the row filters -----------------------------------------------------------------------------------------------------------------
def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if "paeth_tie" in FAULTS:      # ties resolved c, b, a
        return a if pa < pb and pa < pc else b if pb < pc else c
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_row(kind, cur, prev, bpp):
    """cur, prev: lists of the row's and the previous row's ORIGINAL bytes (prev all zero above the image) -> the filtered bytes"""
    out = []
    for i, x in enumerate(cur):
        a = cur[i - bpp] if i >= bpp else 0
        b = prev[i]
        c = prev[i - bpp] if i >= bpp else 0
        pred = (0, a, b, (a + b + ("average_up" in FAULTS)) >> 1, paeth(a, b, c))[kind]
        out.append((x - pred) & 255)
    return out


def row_cost(filtered):
    """the sum of |byte as signed int8|: the PNG specification's heuristic"""
    if "cost_unsigned" in FAULTS:
        return sum(filtered)
    return sum(v if v < 128 else 256 - v for v in filtered)


def choose_filter(cur, prev, bpp):
    """(filter, filtered bytes): the smallest cost, ties to the lowest filter number"""
    rows = [filter_row(k, cur, prev, bpp) for k in range(5)]
    costs = [row_cost(r) for r in rows]
    best = min(costs)
    k = (len(costs) - 1 - costs[::-1].index(best)) if "tie_highest" in FAULTS else costs.index(best)
    return k, rows[k]


def filter_image(img, kind):
    """img uint8 [h, w] or [h, w, bpp]; kind 0 .. 4 or ADAPTIVE -> bytes [h][1 + w * bpp]: filter byte + filtered scanline per row"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    bpp = 1 if img.ndim == 2 else img.shape[2]
    rows = img.reshape(h, w * bpp).tolist()
    out, prev = bytearray(), [0] * (w * bpp)
    for cur in rows:
        k, filtered = choose_filter(cur, prev, bpp) if kind == ADAPTIVE else (kind, filter_row(kind, cur, prev, bpp))
        out.append(k)
        out += bytes(filtered)
        prev = cur
    return bytes(out)


def filter_image_fast(img, kind):
    """the same bytes with numpy, for the larger images of the GPU tests; tests/test_png_encode_reference.py holds it against
    filter_image"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    bpp = 1 if img.ndim == 2 else img.shape[2]
    x = img.reshape(h, w * bpp).astype(np.int32)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    pae = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    all5 = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - pae]) & 255          # [5, h, n]
    if kind == ADAPTIVE:
        cost = np.where(all5 < 128, all5, 256 - all5).sum(axis=2)                 # [5, h]
        pick = np.argmin(cost, axis=0)                                            # the first minimum: the lowest filter number
    else:
        pick = np.full(h, kind)
    rows = all5[pick, np.arange(h)]
    return np.concatenate([pick[:, None], rows], axis=1).astype(np.uint8).tobytes()


# ---- CRC-32 ----------------------------------------------------------------------------------------------------------------------
def crc_table():
    table = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ (POLY if c & 1 else 0)
        table.append(c)
    return table


TABLE = crc_table()


def crc_register(data, reg=0):
    """the table-driven register over `data`, started at `reg`, without the final inversion"""
    for v in data:
        reg = TABLE[(reg ^ v) & 255] ^ (reg >> 8)
    return reg


def gf_mul(a, b):
    """a * b mod P, both reflected (bit 31 is x^0)"""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def x_pow8(nbytes):
    """x^(8 nbytes) mod P by squaring"""
    r, sq, e = 0x80000000, 0x40000000, 8 * nbytes - ("pow_short" in FAULTS and nbytes > 0)
    while e:
        if e & 1:
            r = gf_mul(r, sq)
        sq = gf_mul(sq, sq)
        e >>= 1
    return r


def crc32_pieces(data, cuts):
    """The CRC-32 of `data` from the registers of its pieces data[cuts[k] : cuts[k + 1]], each started at 0: piece k contributes
    reg_k * x^(8 * bytes behind it); the start value 0xFFFFFFFF contributes 0xFFFFFFFF * x^(8 len); then the final inversion."""
    n = len(data)
    edges = [0] + sorted(cuts) + [n]
    total = 0
    for a, b in zip(edges[:-1], edges[1:]):
        total ^= gf_mul(crc_register(data[a:b]), x_pow8(n - b))
    start = 0 if "no_start_term" in FAULTS else gf_mul(0xFFFFFFFF, x_pow8(n))
    return total ^ start ^ 0xFFFFFFFF


# ---- files -----------------------------------------------------------------------------------------------------------------------
def walk(data):
    """[(type, payload, stored CRC, CRC of type + payload)] of a PNG file; asserts the signature and that the chunks fill the file"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, found = 8, []
    while at < len(data):
        assert at + 12 <= len(data), at
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        assert at + 12 + n <= len(data), (kind, n)
        body = data[at + 8:at + 8 + n]
        found.append((kind, body, struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0], zlib.crc32(kind + body)))
        at += 12 + n
    assert at == len(data)
    return found
