"""Decoding inside a baseline JPEG segment with sub-streams -- docs/JPEG_DECODE.md section 1b restated in plain Python, from the
document and independent of csrc/jpeg_entropy.h: states (p, c, k), one step per symbol, recovery of speculative steps, the rounds to
the fixpoint, the counts of blocks that start in a sub-stream, their exclusive scan, the strict pass and the DC sums.  The header
parser, the code table, the bit reader and the sign extension are those of tests/jpeg_sampling_ref.py and tests/jpeg_dec_ref.py,
imported, not edited.  Nothing here imports the package under test.

    coefficients(data, L, faults=(), info=None, simulate=True)
                                                   int16 [MCUs, B, 64] of a whole file, every restart interval decoded by sub-streams
    decode_segment(raw, tables, comp_of, nb, L)    one segment: (int [nb, 64] coefficients, info)

`info` receives per segment: `substreams`, `rounds` (synchronous rounds until nothing changed, the last one included), `distances`
(per guess, in sub-streams: how far the chain from the guess ran before it met the true chain; None: never), `longest_block_bits`.
A round applies every f_i to the states the round before left; f_i is evaluated anew only where its input changed, which gives the
same states.  `faults` plants one deviation by name (FAULTS); tests/test_jpeg_parallel_reference.py shows that each is noticed."""
import numpy as np

import jpeg_sampling_ref as R
from jpeg_dec_ref import _Bits, _code_lookup, _extend

FAULTS = ("equal_by_position", "two_rounds", "dc_saturates", "count_block_ends")
_LOOKUPS = {}


def _lookup(bits, vals):
    """_code_lookup, built once per table"""
    key = (tuple(bits), tuple(vals))
    if key not in _LOOKUPS:
        _LOOKUPS[key] = _code_lookup(bits, vals)
    return _LOOKUPS[key]


class Invalid(Exception):
    """a strict step met an invalid code, a DC category above 11, an index beyond 63 or the segment's end"""


class _Segment:
    def __init__(self, raw, tables, comp_of, nb, L, faults):
        self.bits = _Bits(bytes(raw), ())
        self.tables, self.comp_of, self.B, self.nb, self.L, self.faults = tables, comp_of, len(comp_of), nb, L, faults
        nbytes = self.bits.n // 8
        self.n = max(1, -(-nbytes // L))

    def step(self, state, speculative):
        """one symbol: (the next state, coefficient index or None, value)"""
        p, c, k = state
        bits = self.bits
        (dl, ds), (al, as_) = self.tables[self.comp_of[c]]
        bits.pos = p
        w = bits.window()
        idx, value, nxt, bad = None, 0, 64, p >= bits.n
        if not bad and k == 0:
            n, s = dl[w >> 16], ds[w >> 16]
            bad = n == 0 or s > 11
            if not bad:
                idx, value, nxt, p = 0, _extend(((w << n) & 0xFFFFFFFF) >> (32 - s) if s else 0, s, ()), 1, p + n + s
        elif not bad:
            n, sym = al[w >> 16], as_[w >> 16]
            r, s = sym >> 4, sym & 15
            bad = n == 0 or (s != 0 and k + r > 63)
            if not bad and s == 0:
                nxt, p = (64 if r != 15 else k + 16), p + n
            elif not bad:
                idx, value, nxt, p = k + r, _extend(((w << n) & 0xFFFFFFFF) >> (32 - s), s, ()), k + r + 1, p + n + s
        if bad:
            if not speculative:
                raise Invalid(state)
            p, nxt = p + 1, 64                       # recovery: skip one bit, end the block
        if nxt >= 64:
            return (p, (c + 1) % self.B, 0), idx, value
        return (p, c, nxt), idx, value

    def f(self, i, state):
        """the entry state of sub-stream i + 1 from that of sub-stream i, and the blocks counted on the way"""
        bound, count = 8 * self.L * (i + 1), 0
        if i + 1 == self.n:
            bound = self.bits.n
        while state[0] < bound:
            started = state[2] == 0
            state, _, _ = self.step(state, True)
            if "count_block_ends" in self.faults:
                count += state[2] == 0
            else:
                count += started
        return state, count

    def same(self, a, b):
        return a[0] == b[0] if "equal_by_position" in self.faults else a == b

    def chain(self):
        """the fixpoint itself: e_0 = (0, 0, 0), e_(i+1) = f_i(e_i)"""
        states = [(0, 0, 0)]
        for i in range(self.n - 1):
            states.append(self.f(i, states[i])[0])
        return states

    def entry_states(self):
        """the states by speculation and synchronous rounds, and the number of rounds"""
        n, L = self.n, self.L
        states = [(8 * L * i, 0, 0) for i in range(n)]
        memo = {}
        rounds = 0
        while True:
            rounds += 1
            assert rounds <= n + 1, "the iteration is bounded by the number of sub-streams"
            new, changed = list(states), False
            for i in range(n - 1):
                key = (i, states[i])
                if key not in memo:
                    memo[key] = self.f(i, states[i])[0]
                if not self.same(memo[key], states[i + 1]):
                    new[i + 1], changed = memo[key], True
            states = new
            if not changed or ("two_rounds" in self.faults and rounds == 2):
                break
        return states, rounds

    def decode(self, simulate=True):
        if simulate:
            states, rounds = self.entry_states()
            assert self.faults or states == self.chain(), "the rounds end in the chain from e_0"
        else:
            states, rounds = self.chain(), None
        counts = [self.f(i, states[i])[1] for i in range(self.n)]
        first = [0] * self.n
        for i in range(1, self.n):
            first[i] = first[i - 1] + counts[i - 1]              # the exclusive scan
        out = np.zeros((self.nb, 64), dtype=np.int64)
        end, longest, started_at = None, 0, {}
        for i in range(self.n):                                  # the strict pass: every sub-stream on its own
            state, nxt, cur = states[i], first[i], first[i] - 1
            bound = 8 * self.L * (i + 1) if i + 1 < self.n else None
            if state[2] != 0 and not 0 <= cur < self.nb:
                continue                                         # inside a block behind the segment's last one
            while bound is None or state[0] < bound:
                if state[2] == 0:
                    if nxt >= self.nb:
                        break
                    cur, nxt = nxt, nxt + 1
                    started_at[cur] = state[0]
                state, idx, value = self.step(state, False)
                if idx is not None:
                    assert 0 <= cur < self.nb
                    out[cur, idx] = value
                if state[2] == 0:
                    longest = max(longest, state[0] - started_at.get(cur, state[0]))
                    if nxt == self.nb:
                        end = state[0]
                        break
        if end is None:
            raise Invalid("the chain does not reach the segment's block count")
        if end > self.bits.n or self.bits.n - end > 7:
            raise Invalid("overrun or leftover")
        pred = [0, 0, 0]
        for b in range(self.nb):                                 # DC differences -> predictors, wrapping to int16
            comp = self.comp_of[b % self.B]
            pred[comp] += int(out[b, 0])
            if "dc_saturates" in self.faults:
                out[b, 0] = max(-32768, min(32767, pred[comp]))
            else:
                pred[comp] = ((pred[comp] + 32768) & 0xFFFF) - 32768
                out[b, 0] = pred[comp]
        return out, dict(substreams=self.n, rounds=rounds, states=states, longest_block_bits=longest)

    def distances(self, states):
        """per guess i >= 1: the sub-streams its chain runs before it stands on the true chain (None: never)"""
        true, state = set(), (0, 0, 0)
        while state[0] < self.bits.n:
            true.add(state)
            state, _, _ = self.step(state, True)
        true.add(state)
        out = []
        for i in range(1, self.n):
            state = (8 * self.L * i, 0, 0)
            while state not in true and state[0] < self.bits.n:
                state, _, _ = self.step(state, True)
            out.append((state[0] - 8 * self.L * i) / (8 * self.L) if state in true and state[0] < self.bits.n else None)
        return out


def decode_segment(raw, tables, comp_of, nb, L, faults=(), distances=False, simulate=True):
    seg = _Segment(raw, tables, comp_of, nb, L, faults)
    out, info = seg.decode(simulate)
    if distances:
        info["distances"] = seg.distances(info["states"])
    return out, info


def coefficients(data, L, faults=(), info=None, distances=False, simulate=True):
    """int16 [MCUs, B, 64] in zigzag order; `info` (a list) receives one dict per segment.  simulate=False takes the entry states
    from the chain e_(i+1) = f_i(e_i) directly instead of iterating guesses to it (the rounds are then not counted): the same
    states, without the cost of a stream whose guesses never merge."""
    p = R.parse(data)
    mcus, comp_of = R._schedule(p, ())
    B = len(comp_of)
    tables = [(_lookup(*dc), _lookup(*ac)) for dc, ac in p["huff"]]
    scan = p["scan"]
    raw = np.frombuffer(scan, dtype=np.uint8)
    at = np.flatnonzero((raw[:-1] == 0xFF) & (raw[1:] >= 0xD0) & (raw[1:] <= 0xD7)) if len(raw) > 1 else np.zeros(0, dtype=np.int64)
    starts, ends = [0] + [int(a) + 2 for a in at], [int(a) for a in at] + [len(scan)]
    interval = p["R"] if p["R"] else mcus
    assert len(starts) == -(-mcus // interval)
    out = np.zeros((mcus * B, 64), dtype=np.int64)
    for it, (a, b) in enumerate(zip(starts, ends)):
        m0, m1 = it * interval, min(mcus, (it + 1) * interval)
        seg, seg_info = decode_segment(scan[a:b], tables, comp_of, (m1 - m0) * B, L, faults, distances, simulate)
        out[m0 * B:m1 * B] = seg
        if info is not None:
            info.append(seg_info)
    return out.astype(np.int16).reshape(mcus, B, 64)
