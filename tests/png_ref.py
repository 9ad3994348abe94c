"""A plain-Python restatement of docs/PNG_DECODE.md: inflate (RFC 1950 / 1951) with the status bits of include/dtk.h, the Adler-32,
and the five PNG row filters.  It is what the GPU tests compare statuses with and what the CPU tests hold against zlib and Pillow; it
shares no code with the library.  `FAULTS` plants single mistakes that tests/test_png_reference.py must notice."""
import struct
import zlib

import numpy as np

S_HEADER, S_BTYPE, S_STORED, S_TABLE, S_CODE, S_DISTANCE, S_OVERRUN, S_LENGTH, S_ADLER, S_STREAM = (1 << k for k in range(10))
PNG_S_FILTER = 1024

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in range(2)]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CLEN, LITLEN, DIST = 0, 1, 2

# planted faults (tests): a set of names
FAULTS = set()


class Fault(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


class Bits:
    """LSB-first; bits beyond the end read as zero, and `check` raises OVERRUN once the position has passed the end"""

    def __init__(self, data):
        self.data = bytes(data) + bytes(8)
        self.avail = 8 * len(data)
        self.pos = 0

    def peek(self, n):      # n <= 32
        at = self.pos >> 3
        if at + 8 > len(self.data):
            return 0
        return (int.from_bytes(self.data[at:at + 8], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n)
        self.pos += n
        return v

    def take_msb(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.take(1)
        return v

    def check(self):
        if self.pos > self.avail:
            raise Fault(S_OVERRUN)


class Code:
    """a canonical code from its lengths: {(length, code): symbol}; raises Fault(S_TABLE) as inf_code_sort does"""

    def __init__(self, lens, kind):
        count = [0] * 16
        for v in lens:
            count[v] += 1
        left = 1
        for length in range(1, 16):
            left = (left << 1) - count[length]
            if left < 0:
                raise Fault(S_TABLE)
        coded = len(lens) - count[0]
        if left > 0 and not (kind == DIST and (coded == 0 or (coded == 1 and count[1] == 1))):
            raise Fault(S_TABLE)
        if kind == LITLEN and (len(lens) <= 256 or lens[256] == 0):
            raise Fault(S_TABLE)
        self.table, code = {}, 0
        self.maxlen = max([0] + [v for v in lens])
        for length in range(1, 16):
            for sym, v in enumerate(lens):
                if v == length:
                    self.table[(length, code)] = sym
                    code += 1
            code <<= 1

    def decode(self, bits, longest, stats=None):
        """one symbol; no match: OVERRUN when fewer than `longest` bits remain, else CODE"""
        code, window = 0, bits.peek(15)
        for length in range(1, 16):
            code = (code << 1) | ((window >> (length - 1)) & 1)
            sym = self.table.get((length, code))
            if sym is not None:
                bits.pos += length
                bits.check()
                if stats is not None:
                    stats["longest_code"] = max(stats["longest_code"], length)
                return sym
        raise Fault(S_OVERRUN if bits.pos + longest > bits.avail else S_CODE)


def fixed_lens():
    return [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32


def read_dynamic(bits):
    hlit, hdist, hclen = 257 + bits.take(5), 1 + bits.take(5), 4 + bits.take(4)
    bits.check()
    if hlit > 286 or hdist > 30:
        raise Fault(S_TABLE)
    cl = [0] * 19
    for i in range(hclen):
        cl[CLEN_ORDER[i]] = bits.take(3)
    bits.check()
    code = Code(cl, CLEN)
    lens, total = [], hlit + hdist
    while len(lens) < total:
        sym = code.decode(bits, 7)
        if sym < 16:
            lens.append(sym)
            continue
        val = 0
        if sym == 16:
            rep = 3 + bits.take(2)
            bits.check()
            if not lens:
                raise Fault(S_TABLE)
            val = 0 if "repeat16_zero" in FAULTS else lens[-1]
        elif sym == 17:
            rep = 3 + bits.take(3)
        else:
            rep = 11 + bits.take(7)
        bits.check()
        if len(lens) + rep > total:
            raise Fault(S_TABLE)
        lens += [val] * rep
    return lens[:hlit], lens[hlit:]


def inflate(data, expected, wrapper=True):
    """-> (bytes of length `expected` -- what was decoded before the first fault, then zeros --, status, stats).  stats: the
    longest code and the largest distance seen, the number of blocks by type and of tokens (literals, matches, block ends)."""
    stats = {"longest_code": 0, "largest_distance": 0, "blocks": [0, 0, 0], "tokens": 0}
    out = bytearray()
    status = 0
    bits = Bits(data)
    try:
        if wrapper:
            cmf, flg = bits.take(8), bits.take(8)
            bits.check()
            if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 or (flg & 32):
                raise Fault(S_HEADER)
        while True:
            last, btype = bits.take(1), bits.take(2)
            bits.check()
            if btype == 3:
                raise Fault(S_BTYPE)
            stats["blocks"][btype] += 1
            if btype == 0:
                bits.pos += (8 - bits.pos % 8) % 8
                n, nn = bits.take(16), bits.take(16)
                bits.check()
                if n ^ nn != 0xFFFF:
                    raise Fault(S_STORED)
                if n > expected - len(out):
                    raise Fault(S_LENGTH)
                have = max(0, bits.avail - bits.pos) // 8
                at = bits.pos // 8
                out += data[at:at + min(n, have)]
                bits.pos += 8 * min(n, have)
                if have < n:
                    raise Fault(S_OVERRUN)
            else:
                ll, dl = fixed_lens() if btype == 1 else read_dynamic(bits)
                lit = Code(ll, LITLEN)      # both codes are examined before anything is decoded: a TABLE fault of either
                dist = Code(dl, DIST)
                while True:
                    sym = lit.decode(bits, 15, stats)
                    stats["tokens"] += 1
                    if sym < 256:
                        if len(out) >= expected:
                            raise Fault(S_LENGTH)
                        out.append(sym)
                        continue
                    if sym == 256:
                        break
                    if sym > 285:
                        raise Fault(S_CODE)
                    k = sym - 257
                    length = LENGTH_BASE[k] + ("length_base" in FAULTS and k == 9) + bits.take(LENGTH_EXTRA[k])
                    dist_sym = dist.decode(bits, 15, stats)
                    if dist_sym > 29:
                        raise Fault(S_CODE)
                    extra = DIST_EXTRA[dist_sym]
                    d = DIST_BASE[dist_sym] + (bits.take_msb(extra) if "dist_extra_msb" in FAULTS else bits.take(extra))
                    bits.check()
                    stats["largest_distance"] = max(stats["largest_distance"], d)
                    if d > len(out):
                        raise Fault(S_DISTANCE)
                    if length > expected - len(out):
                        raise Fault(S_LENGTH)
                    for _ in range(length):
                        out.append(out[-d])
            if last:
                break
        if len(out) != expected:
            raise Fault(S_LENGTH)
        if wrapper and len(data) - (bits.pos + 7) // 8 < 4:
            raise Fault(S_OVERRUN)
    except Fault as fault:
        status = fault.status
    body = bytes(out[:expected]) + bytes(max(0, expected - len(out)))
    if wrapper and status == 0 and adler32(body) != struct.unpack(">I", data[-4:])[0]:
        status = S_ADLER
    return body, status, stats


def adler32(data):
    """RFC 1950 section 9, byte by byte"""
    s1, s2 = 1, 0
    for v in data:
        s1 = (s1 + v) % 65521
        s2 = (s2 + s1) % 65521
    return (s2 << 16) | s1


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if "paeth_tie" in FAULTS:      # ties resolved c, b, a (a against b never shows: pa == pb <= pc forces a == b)
        return a if pa < pb and pa < pc else b if pb < pc else c
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter(raw, h, w, bpp):
    """raw: bytes [h][1 + w * bpp] -> (uint8 [h, w, bpp], status)"""
    pitch, status = 1 + w * bpp, 0
    out = np.zeros((h, w * bpp), dtype=np.uint8)
    prev = [0] * (w * bpp)
    for y in range(h):
        f, line = raw[y * pitch], raw[y * pitch + 1:(y + 1) * pitch]
        if f > 4:
            status, f = PNG_S_FILTER, 0
        cur = [0] * (w * bpp)
        for i, v in enumerate(line):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b + ("average_up" in FAULTS)) >> 1, paeth(a, b, c))[f]
            cur[i] = (v + pred) & 255
        out[y] = cur
        prev = cur
    return out.reshape(h, w, bpp), status


# ---- files -----------------------------------------------------------------------------------------------------------------------
def chunks(data):
    """[(type, payload)] of a PNG file, CRCs checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, found = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), kind
        found.append((kind, body))
        at += 12 + n
    return found


def palette_to_l(plte):
    """what Pillow's convert("L") makes of a palette: ITU-R 601-2 luma in 16-bit fixed point -> uint8 [256], zero beyond the palette"""
    lut = np.zeros(256, dtype=np.uint8)
    for i in range(len(plte) // 3):
        r, g, b = plte[3 * i:3 * i + 3]
        lut[i] = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    return lut


def decode_png(data):
    """an 8-bit non-interlaced file of colour type 0, 2 or 3 -> (uint8 [h, w, bpp] -- palette INDICES for type 3 --, status, stats,
    the PLTE payload or None)"""
    found = chunks(data)
    w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", found[0][1])
    assert found[0][0] == b"IHDR" and depth == 8 and ctype in (0, 2, 3) and (comp, flt, lace) == (0, 0, 0)
    bpp = 3 if ctype == 2 else 1
    stream = b"".join(body for kind, body in found if kind == b"IDAT")
    raw, status, stats = inflate(stream, h * (1 + w * bpp))
    px, fstatus = unfilter(raw, h, w, bpp)
    plte = [body for kind, body in found if kind == b"PLTE"]
    return px, status | fstatus, stats, plte[0] if plte else None
