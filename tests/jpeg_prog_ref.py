"""Progressive (SOF2) JPEG entropy decoding restated in plain Python from docs/JPEG_DECODE.md, section "Progressive files": the four
scan kinds of T.81 Annex G, the block order of interleaved and one-component scans, restart segments.  The canonical code table, the
bit reader and the sign extension are tests/jpeg_dec_ref.py's; the MCU geometry is tests/jpeg_sampling_ref.py's.  Nothing here imports
the package under test.

    parse(data)                              H, W, sampling, qt [C, 64], adobe, R, scans: [dict(comps, Ss, Se, Ah, Al, huff, R, body)]
    coefficients(data, faults=(), info=None) int16 [MCUs, B, 64], zigzag order, the MCU-major layout of the baseline decoder

The oracle is *progressive coefficients = baseline coefficients of the same picture and settings* (jpeg_sampling_ref.coefficients).
`faults` plants one deviation by name (FAULTS); `info` (a dict) receives `eob_categories`, the set of end-of-band run categories met
per scan kind ("first", "refine")."""
import numpy as np

from jpeg_dec_ref import _Bits, _code_lookup, _extend
from jpeg_sampling_ref import FACTORS, GRAY, LUMA, blocks_per_mcu, mcu_grid

FAULTS = ("padded_grid", "cb_cr_swapped", "refine_run_off_by_one", "run_skips_corrections",
          "placed_before_zeros", "al_dropped")


def parse(data):
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    i, dqt, dht, R, sof, adobe, scans = 2, {}, {}, 0, None, None, []
    while True:
        assert data[i] == 0xFF, f"no marker at {i}"
        marker = data[i + 1]
        if marker == 0xD9:
            break
        length = int.from_bytes(data[i + 2:i + 4], "big")
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
        assert marker != 0xC0, "not progressive"
        if marker == 0xC2:
            assert seg[0] == 8 and seg[5] in (1, 3)
            sof = seg
        if marker == 0xDA:
            n = seg[0]
            comps = [seg[1 + 2 * c] - 1 for c in range(n)]
            Ss, Se, Ah, Al = seg[1 + 2 * n], seg[2 + 2 * n], seg[3 + 2 * n] >> 4, seg[3 + 2 * n] & 15
            huff = [(dht.get(seg[2 + 2 * c] >> 4), dht.get(0x10 | (seg[2 + 2 * c] & 15))) for c in range(n)]
            j = i                       # the body ends at the first marker that is neither stuffing nor RSTn
            while not (data[j] == 0xFF and data[j + 1] != 0 and not 0xD0 <= data[j + 1] <= 0xD7):
                j += 1
            scans.append(dict(comps=comps, Ss=Ss, Se=Se, Ah=Ah, Al=Al, huff=huff, R=R, body=data[i:j]))
            i = j
    H, W, n = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big"), sof[5]
    cs = [tuple(sof[6 + 3 * c:9 + 3 * c]) for c in range(n)]
    assert [c[0] for c in cs] == [1, 2, 3][:n], cs
    sampling = GRAY if n == 1 else FACTORS[tuple(c[1] for c in cs)]
    return dict(H=H, W=W, sampling=sampling, qt=np.stack([dqt[c[2]] for c in cs]), adobe=adobe, R=R, scans=scans)


_LOOKUPS = {}


def _lookup(table):
    """jpeg_dec_ref._code_lookup of a (bits, vals) table, built once per distinct table"""
    key = (tuple(table[0]), tuple(table[1]))
    if key not in _LOOKUPS:
        if len(_LOOKUPS) > 256:
            _LOOKUPS.clear()
        _LOOKUPS[key] = _code_lookup(*table)
    return _LOOKUPS[key]


def _split(body):
    """the restart segments of a scan body"""
    raw = np.frombuffer(body, dtype=np.uint8)
    at = np.flatnonzero((raw[:-1] == 0xFF) & (raw[1:] >= 0xD0) & (raw[1:] <= 0xD7)) if len(raw) > 1 else np.zeros(0, dtype=np.int64)
    return [body[a:b] for a, b in zip([0] + [int(a) + 2 for a in at], [int(a) for a in at] + [len(body)])]


def component_grid(H, W, sampling, comp, padded=False):
    """(block rows, block columns) of a component: the REAL grid a one-component scan walks, or the MCU padding"""
    mh, mw = mcu_grid(H, W, sampling)
    v, h = (1 + max(b[0] for b in LUMA[sampling]), 1 + max(b[1] for b in LUMA[sampling]))
    if padded:
        return (mh * v, mw * h) if comp == 0 else (mh, mw)
    if comp == 0:
        return -(-H // 8), -(-W // 8)
    return -(-(-(-H // v)) // 8), -(-(-(-W // h)) // 8)


def _place(sampling, comp, by, bx, mw):
    """(MCU, block of the MCU) of block (by, bx) of a component"""
    if comp:
        return by * mw + bx, len(LUMA[sampling]) + comp - 1
    v, h = (1 + max(b[0] for b in LUMA[sampling]), 1 + max(b[1] for b in LUMA[sampling]))
    return (by // v) * mw + bx // h, (by % v) * h + bx % h


def _bit(bits):
    v = bits.window() >> 31
    bits.pos += 1
    return v


def _correct(out, pos, bits, Al):
    """one correction bit for an already non-zero coefficient"""
    if _bit(bits) and not (int(out[pos]) & (1 << Al)):
        out[pos] += (1 << Al) if out[pos] > 0 else -(1 << Al)


def coefficients(data, faults=(), info=None):
    p = parse(data)
    s = p["sampling"]
    mh, mw = mcu_grid(p["H"], p["W"], s)
    B = blocks_per_mcu(s)
    comp_of = [0] * len(LUMA[s]) + ([] if s == GRAY else [1, 2])
    out = np.zeros((mh * mw, B, 64), dtype=np.int64)
    seen = {"first": set(), "refine": set()}
    for scan in p["scans"]:
        Ss, Se, Ah, Al = scan["Ss"], scan["Se"], scan["Ah"], scan["Al"]
        shift = 0 if "al_dropped" in faults else Al
        comps = scan["comps"]
        if "cb_cr_swapped" in faults and len(comps) == 1 and comps[0]:
            comps = [3 - comps[0]]
        # the scan's blocks in decoding order: (component slot of the scan, MCU, block of the MCU)
        if len(comps) > 1:
            assert comps == [0, 1, 2] and Ss == 0
            order = [[(comp_of[k], m, k) for k in range(B)] for m in range(mh * mw)]       # one unit = one MCU
        else:
            rows, cols = component_grid(p["H"], p["W"], s, comps[0], padded="padded_grid" in faults)
            order = [[(0,) + _place(s, comps[0], by, bx, mw)] for by in range(rows) for bx in range(cols)]
        segments = _split(scan["body"])
        R = scan["R"] if scan["R"] else len(order)     # the interval in force at the scan's SOS
        assert len(segments) == -(-len(order) // R), (len(segments), len(order), R)
        run = 0
        for it, raw in enumerate(segments):
            bits = _Bits(raw, ())
            pred = [0, 0, 0]
            run = 0                     # (an encoder ends every run before a restart marker: keeping it would go unnoticed)
            for unit in order[it * R:(it + 1) * R]:
                for slot, m, k in unit:
                    blk = out[m, k]
                    if Ss == 0 and Ah == 0:                                   # DC first
                        dl, ds = _lookup(scan["huff"][slot][0])
                        w = bits.window()
                        n, c = dl[w >> 16], ds[w >> 16]
                        assert n, "no DC code matches"
                        pred[slot] += _extend(((w << n) & 0xFFFFFFFF) >> (32 - c) if c else 0, c, ())
                        bits.pos += n + c
                        blk[0] = pred[slot] << shift
                    elif Ss == 0:                                             # DC refinement
                        if _bit(bits):
                            blk[0] |= 1 << shift
                    elif Ah == 0:                                             # AC first
                        if run:
                            run -= 1
                            continue
                        al, as_ = _lookup(scan["huff"][0][1])
                        i = Ss
                        while i <= Se:
                            w = bits.window()
                            n, sym = al[w >> 16], as_[w >> 16]
                            assert n, "no AC code matches"
                            r, c = sym >> 4, sym & 15
                            bits.pos += n
                            if c:
                                i += r
                                assert i <= Se, "a run beyond the band"
                                blk[i] = _extend(((w << n) & 0xFFFFFFFF) >> (32 - c), c, ()) << shift
                                bits.pos += c
                                i += 1
                            elif r == 15:
                                i += 16
                            else:
                                seen["first"].add(r)
                                run = (1 << r) + ((((w << n) & 0xFFFFFFFF) >> (32 - r)) if r else 0) - 1
                                bits.pos += r
                                break
                    else:                                                     # AC refinement
                        al, as_ = _lookup(scan["huff"][0][1])
                        i = Ss
                        if run == 0:
                            while i <= Se:
                                w = bits.window()
                                n, sym = al[w >> 16], as_[w >> 16]
                                assert n, "no AC code matches"
                                r, c = sym >> 4, sym & 15
                                bits.pos += n
                                value = 0
                                if c:
                                    assert c == 1, "a refinement size other than 1"
                                    value = (1 << shift) if _bit(bits) else -(1 << shift)
                                elif r != 15:
                                    seen["refine"].add(r)
                                    run = (1 << r) + ((((w << n) & 0xFFFFFFFF) >> (32 - r)) if r else 0)
                                    if "refine_run_off_by_one" in faults:
                                        run -= 1
                                    bits.pos += r
                                    break
                                if "placed_before_zeros" in faults and value:
                                    while blk[i]:
                                        _correct(blk, i, bits, shift)
                                        i += 1
                                    r = 0
                                # pass r still-zero positions; the next still-zero one takes the value (or ends a 16-skip)
                                while i <= Se:
                                    if blk[i]:
                                        _correct(blk, i, bits, shift)
                                    else:
                                        r -= 1
                                        if r < 0:
                                            break
                                    i += 1
                                assert i <= Se, "a run beyond the band"
                                if value:
                                    blk[i] = value
                                i += 1
                        if run:
                            if "run_skips_corrections" not in faults:
                                while i <= Se:
                                    if blk[i]:
                                        _correct(blk, i, bits, shift)
                                    i += 1
                            run -= 1
            assert bits.pos <= bits.n and bits.n - bits.pos <= 7, "the stream does not fit the schedule"
            assert run == 0 or "refine_run_off_by_one" in faults, "a run beyond the segment"
    if info is not None:
        info["eob_categories"] = seen
    return out.astype(np.int16)
