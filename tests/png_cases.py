"""Inputs for the PNG decoder's tests (pure Python / numpy): a minimal PNG writer that applies a CHOSEN filter to every row (Pillow
cannot be told which to use) and splits the IDAT where it is told; hand-built DEFLATE streams for what zlib never emits (distances
up to 32 768, damaged headers); the list of valid streams and the list of damaged ones with the status each must produce."""
import functools
import random
import struct
import zlib

import numpy as np

import png_ref as R

SIGNATURE = b"\x89PNG\r\n\x1a\n"


# ---- PNG files --------------------------------------------------------------------------------------------------------------------
def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def filter_rows(array, filters):
    """array uint8 [h, w] or [h, w, 3]; filters: one type for all rows or one per row -> bytes [h][1 + w * bpp]"""
    a = np.asarray(array, dtype=np.uint8)
    h, w = a.shape[:2]
    bpp = 1 if a.ndim == 2 else a.shape[2]
    rows = a.reshape(h, w * bpp).astype(np.int32)
    types = [filters] * h if isinstance(filters, int) else list(filters)
    assert len(types) == h
    out = bytearray()
    zero = np.zeros(w * bpp, dtype=np.int32)
    for y in range(h):
        x, b = rows[y], rows[y - 1] if y else zero
        left = np.concatenate((zero[:bpp], x[:-bpp])) if w * bpp > bpp else zero[:w * bpp]
        upleft = np.concatenate((zero[:bpp], b[:-bpp])) if w * bpp > bpp else zero[:w * bpp]
        t = types[y]
        if t == 0 or t > 4:
            pred = zero
        elif t == 1:
            pred = left
        elif t == 2:
            pred = b
        elif t == 3:
            pred = (left + b) >> 1
        else:
            p = left + b - upleft
            pa, pb, pc = np.abs(p - left), np.abs(p - b), np.abs(p - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, b, upleft))
        out.append(t)
        out += ((x - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def write_png(array, filters=0, idat_split=(), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, palette=None, extra=()):
    """array uint8 [h, w] (grey, or palette indices when `palette` -- bytes, 3 per entry -- is given) or [h, w, 3].  idat_split: byte
    positions of the compressed stream at which a new IDAT chunk starts (0, or a repeated position, makes an empty chunk).  extra:
    chunks (kind, body) placed before the first IDAT."""
    a = np.asarray(array, dtype=np.uint8)
    h, w = a.shape[:2]
    ctype = 3 if palette is not None else 0 if a.ndim == 2 else 2
    comp = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    stream = comp.compress(filter_rows(a, filters)) + comp.flush()
    cuts = [0] + [min(int(p), len(stream)) for p in idat_split] + [len(stream)]
    data = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0))
    if palette is not None:
        data += chunk(b"PLTE", bytes(palette))
    for kind, body in extra:
        data += chunk(kind, body)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        data += chunk(b"IDAT", stream[lo:hi])
    return data + chunk(b"IEND", b"")


def picture(h, w, channels=3, seed=0):
    """smooth enough that every filter has something to predict, noisy enough that no filter makes it trivial"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = (3 * x + 5 * y)[..., None] + np.arange(channels) * 40
    img = (base + rng.integers(0, 24, size=(h, w, channels))) & 255
    return img.astype(np.uint8) if channels > 1 else img[..., 0].astype(np.uint8)


def filter_sequence(h, seed=0):
    """a filter per row such that, over 26 rows or more, every filter follows every other (and itself): the 25 ordered pairs in a
    seeded order, as an Eulerian walk; shorter images take its start"""
    rng = random.Random(seed)
    edges = {a: [b for b in range(5)] for a in range(5)}
    for a in edges:
        rng.shuffle(edges[a])
    stack, walk = [rng.randrange(5)], []
    while stack:                       # Hierholzer on the complete digraph with loops
        v = stack[-1]
        if edges[v]:
            stack.append(edges[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == 26 and len(set(zip(walk[:-1], walk[1:]))) == 25
    return [walk[i % 25] for i in range(h)]


# ---- DEFLATE by hand ------------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):            # LSB first
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, n):            # a Huffman code: MSB first
        for k in range(n - 1, -1, -1):
            self.bits((value >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


def fixed_litlen(w, sym):
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xC0 + sym - 280, 8)


def fixed_tokens(w, tokens):
    """tokens: ints (literals), (length, distance) pairs, ("litlen", symbol) or ("dist", length, distance symbol) for raw symbols"""
    for t in tokens:
        if isinstance(t, int):
            fixed_litlen(w, t)
        elif t[0] == "litlen":
            fixed_litlen(w, t[1])
        else:
            length, dist_sym, dist_extra = (t[1], t[2], 0) if t[0] == "dist" else (t[0], None, 0)
            k = max(i for i, b in enumerate(R.LENGTH_BASE) if b <= length)
            fixed_litlen(w, 257 + k)
            w.bits(length - R.LENGTH_BASE[k], R.LENGTH_EXTRA[k])
            if dist_sym is None:
                dist_sym = max(i for i, b in enumerate(R.DIST_BASE) if b <= t[1])
                dist_extra = t[1] - R.DIST_BASE[dist_sym]
            w.code(dist_sym, 5)
            if dist_sym < 30:
                w.bits(dist_extra, R.DIST_EXTRA[dist_sym])


def deflate_fixed(tokens, final=True):
    """one fixed-Huffman block (raw DEFLATE) from explicit tokens"""
    w = BitWriter()
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    fixed_tokens(w, tokens)
    fixed_litlen(w, 256)
    return w.done()


def stored(data, nlen_xor=0xFFFF):
    """stored blocks (raw DEFLATE), at most 65 535 bytes each"""
    out, pieces = bytearray(), [data[i:i + 65535] for i in range(0, len(data), 65535)] or [b""]
    for k, piece in enumerate(pieces):
        out += bytes([1 if k == len(pieces) - 1 else 0]) + struct.pack("<HH", len(piece), len(piece) ^ nlen_xor) + piece
    return bytes(out)


def wrap(raw, data):
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data))


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def compress(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


def fibonacci_bytes(n=22, seed=5):
    """bytes whose n values have Fibonacci frequencies: an optimal prefix code for them is n - 1 deep, which zlib caps at 15"""
    a, b, data = 1, 1, bytearray()
    for v in range(n):
        data += bytes([v * 7 + 3]) * a
        a, b = b, a + b
    items = list(data)
    random.Random(seed).shuffle(items)
    return bytes(items)


def text_like(n=70000, seed=9):
    rng = random.Random(seed)
    words = ["".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(2, 11))) for _ in range(300)]
    phrases = [" ".join(rng.choice(words) for _ in range(rng.randint(20, 60))) for _ in range(12)]
    out = []
    size = 0
    while size < n:
        s = rng.choice(phrases) if rng.random() < 0.3 else rng.choice(words)
        out.append(s)
        size += len(s) + 1
    return " ".join(out).encode()[:n]


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, zlib stream, the bytes it holds)]: every one valid"""
    rng_lits = list(random_bytes(32768 + 300, 3))
    found = []

    def add(name, stream, data):
        found.append((name, stream, bytes(data)))

    add("empty", compress(b""), b"")
    add("one_byte", compress(b"\x5a"), b"\x5a")
    big = random_bytes(70001, 1)
    add("level0_two_stored_blocks", compress(big, 0), big)
    smooth = bytes((i // 3 + (i % 7)) & 255 for i in range(20000))
    add("z_fixed", compress(smooth, 6, zlib.Z_FIXED), smooth)
    add("default_dynamic", compress(smooth + big[:3000]), smooth + big[:3000])
    fib = fibonacci_bytes()
    add("huffman_only_fibonacci", compress(fib, 6, zlib.Z_HUFFMAN_ONLY), fib)
    add("full_flush_in_the_middle", compress(smooth[:9001], 6, flush_at=4001), smooth[:9001])
    const = bytes([77]) * 5000
    add("z_rle_constant", compress(const, 6, zlib.Z_RLE), const)
    for name, tokens in (("hand_length3_distance1", [97, (3, 1)]),
                         ("hand_distance_32768", rng_lits[:32768] + [(258, 32768)]),
                         ("hand_match_crosses_the_ring_wrap", rng_lits[:32768 - 100] + [(258, 5000), (258, 300), (200, 32768), (258, 7)]),
                         ("hand_period_shorter_than_length", [1, 2, 3, (258, 3), (100, 2), 9, (258, 5)])):
        data = expand(tokens)
        add(name, wrap(deflate_fixed(tokens), data), data)
    add("hand_stored", wrap(stored(big[:700]), big[:700]), big[:700])
    text = text_like()
    add("text_like_long_matches", compress(text, 9), text)
    return found


@functools.lru_cache(maxsize=None)
def damaged():
    """[(name, zlib stream, expected output bytes, the status it must produce, whether zlib.decompress raises on it)]"""
    found = []
    smooth = bytes((i // 3 + (i % 7)) & 255 for i in range(20000))
    good = compress(smooth + random_bytes(3000, 1))
    n = len(smooth) + 3000
    for cut in (1, 2, 3, 11, 40, len(good) // 2, len(good) - 5, len(good) - 1):
        found.append((f"truncated_to_{cut}_bytes", good[:cut], n, R.S_OVERRUN, True))
    st = wrap(stored(smooth[:500]), smooth[:500])
    found.append(("truncated_stored", st[:300], 500, R.S_OVERRUN, True))
    found.append(("block_type_3", wrap(b"\x07" + bytes(8), b""), 16, R.S_BTYPE, True))
    found.append(("len_nlen_mismatch", wrap(stored(smooth[:100], 0xFFFE), smooth[:100]), 100, R.S_STORED, True))
    found.append(("litlen_symbol_286", wrap(deflate_fixed([65, 66, ("litlen", 286), 67]), b"AB"), 8, R.S_CODE, True))
    found.append(("distance_symbol_30", wrap(deflate_fixed([65, 66, 67, ("dist", 3, 30), 68]), b"ABC"), 8, R.S_CODE, True))
    w = BitWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(30, 5), w.bits(0, 5), w.bits(0, 4)
    found.append(("hlit_287", wrap(w.done() + bytes(8), b""), 8, R.S_TABLE, True))
    w = BitWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(0, 5), w.bits(0, 5), w.bits(0, 4)
    for _ in range(4):
        w.bits(1, 3)           # four code-length codes of one bit
    found.append(("oversubscribed_code_lengths", wrap(w.done() + bytes(8), b""), 8, R.S_TABLE, True))
    w = BitWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(0, 5), w.bits(0, 5), w.bits(1, 4)
    for v in (0, 0, 0, 1, 1):  # code-length code: '0' = length 0, '1' = length 8
        w.bits(v, 3)
    for _ in range(256):
        w.bits(1, 1)           # literals 0 .. 255: eight bits each, a complete code
    w.bits(0, 1), w.bits(0, 1)  # no code for 256, no distance code
    found.append(("no_end_of_block_code", wrap(w.done() + bytes(8), b""), 8, R.S_TABLE, True))
    found.append(("wrong_adler_trailer", good[:-1] + bytes([good[-1] ^ 1]), n, R.S_ADLER, True))
    found.append(("output_one_byte_longer", good, n - 1, R.S_LENGTH, False))
    found.append(("output_one_byte_shorter", good, n + 1, R.S_LENGTH, False))
    found.append(("fdict_set", b"\x78\x20" + good[2:], n, R.S_HEADER, True))
    lits = list(random_bytes(32767, 3))
    tokens = lits + [(258, 32768)]
    found.append(("distance_32768_after_32767_literals", wrap(deflate_fixed(tokens), bytes(lits)), 32767 + 258, R.S_DISTANCE, True))
    return found
