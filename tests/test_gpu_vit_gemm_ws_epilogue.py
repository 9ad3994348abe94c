"""-m gpu: the hand-cut step of gemm_ws_kernel (csrc/vit_gemm_ws.h: peeled first steps and tail, branch-free steady state, the previous
tile's epilogue in slots between the MFMAs, flush reads issued together) against the untouched round 1-3 form of the same kernel
(DTK_VIT_GEMM_WS_V1).  Both forms evaluate the same expressions in the same MFMA order, so on the same operands every output BIT
must agree -- guard bands and, for the QKV layouts, the zero padding rows S .. Sp included.

Row counts: 1, 31, 32, 33, 64, 65, 113 (one to four tiles in a chunk of one: the tail alone; odd / even / ragged) and the counts of
tests/vit_gemm_ref.py ws_rows_for that give 2, 3 and >= 5 tiles per chunk with a short last chunk -- the peeled pair alone, the
peeled pair + the odd tail, and the steady-state loop.  QKV: frames of S = 21 x 7 (several frames shorter than a tile: the
launcher sends these to the tiled kernel under either flag), 37 x 3, 222 x 3 and a multi-chunk count of each S, so frame ends fall inside
a tile and inside a 4-row fragment.  N = 1152 and N = 384 leave waves without columns in the last column group: whatever they
stored would land in the next row or the guard band and break the equality."""
import pytest
import torch

import vit_gemm_ref as R
from test_gpu_vit_gemm import BF16, DEV, F16, WS_V1, run_stage

pytestmark = pytest.mark.gpu

D = 384
ROLES = {"qkv": R.QKV, "proj": R.PROJ, "fc1": R.FC1}


def sp_of(s):
    return -(-s // 64) * 64


def cases(role):
    """[(rows, S, Sp)]; S = 0 outside QKV."""
    N, _ = R.shape(role, D)
    if role != R.QKV:
        rows = [1, 31, 32, 33, 64, 65, 113] + [R.ws_rows_for(N, lo, hi) for lo, hi in ((2, 2), (3, 3), (5, 99))]
        return [(r, 0, 0) for r in rows]
    out = [(7 * 21, 21, 64), (3 * 37, 37, 64), (3 * 222, 222, 256)]
    for s, lo, hi in ((21, 5, 99), (37, 5, 99), (222, 2, 2), (222, 3, 3), (222, 5, 99)):
        r = R.ws_rows_for(N, lo, hi, step=s)
        nch, tpc, last = R.ws_grid(N, r)
        assert nch > 1 and lo <= tpc <= hi and 0 < last < tpc and r % s == 0, (r, s, nch, tpc, last)
        out.append((r, s, sp_of(s)))
    return out


def operands(role, dtype, rows, S, Sp, seed):
    o = R.make_real(role, D, rows, dtype, seed, device=DEV)
    if role == R.QKV:
        o["S"], o["Sp"] = S, Sp
    return o


def bits(t):
    return t.contiguous().view(torch.int16)


def assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        ne = bits(a[k]) != bits(b[k])
        assert not bool(ne.any()), f"{what}: {int(ne.sum())} elements of {k} differ, first at flat index {int(ne.flatten().nonzero()[0])}"


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("role", list(ROLES))
def test_bitwise_against_v1(role, dt):
    """Flags 0 (the hand-cut form) and DTK_VIT_GEMM_WS_V1 on the same operands: identical bits.  run_stage asserts every guard band."""
    dtype = F16 if dt == "fp16" else BF16
    r = ROLES[role]
    for i, (rows, S, Sp) in enumerate(cases(r)):
        o = operands(r, dtype, rows, S, Sp, 4241 + 17 * i + 1000 * r + (dt == "bf16"))
        new, old = run_stage(o, 0), run_stage(o, WS_V1)
        assert_same_bits(new, old, f"{role} {dt} rows={rows} S={S}")
        if r == R.QKV:
            assert R.qkv_padding_is_zero(new["q"], new["k"], new["vt"], S), f"{role} {dt} rows={rows} S={S}: padding rows written"
    print(f"gemm_ws epilogue {role} {dt}: {len(cases(r))} row counts bit-equal to the V1 form")


@pytest.mark.parametrize("role", list(ROLES))
def test_repeatable(role):
    """The same launch three times into fresh outputs: equal bits (an instruction-order hazard shows as tokens that change from run to run).
    The case with >= 5 tiles per chunk: peeled steps, steady state and tail."""
    r = ROLES[role]
    rows, S, Sp = cases(r)[-1]
    o = operands(r, F16, rows, S, Sp, 977 + r)
    first = run_stage(o, 0)
    for rep in (1, 2):
        assert_same_bits(run_stage(o, 0), first, f"{role} rows={rows} run {rep}")


@pytest.mark.parametrize("role", [R.QKV, R.FC1], ids=["qkv", "fc1"])
def test_overflow_word_in_steady_state(role):
    """GemmEpi::ovf through the slots of a steady-state step: one stored value of 65536 (256 products of 16 x 16) in the third tile of a
    chunk of >= 5 tiles, last column, sets bit 2 (QKV) / 4 (fc1) and is stored as the saturated 65504; 255 products (65280) leave the
    word at 0."""
    N, K = R.shape(role, D)
    rows = R.ws_rows_for(N, 5, 99)
    assert R.ws_grid(N, rows)[1] >= 5
    row = 2 * 32 + 5
    bit = 2 if role == R.QKV else 4
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    for terms, want_word, want in ((256, bit, 65504.0), (255, 0, 65280.0)):
        A, W = torch.zeros(rows, K, device=DEV), torch.zeros(N, K, device=DEV)
        A[row, :terms] = 16.0
        W[N - 1, :256] = 16.0
        o = {"role": role, "D": D, "rows": rows, "dtype": F16, "split": False, "w_scale": 1.0, "exact": False, "S": rows, "Sp": sp_of(rows),
             "A": A.to(F16), "W": W.to(F16), "bias": torch.zeros(N, device=DEV)}
        word.zero_()
        got = run_stage(o, 0, ovf=word)
        stored = float(R.matrix(o, got)[row, N - 1])
        assert int(word) == want_word and stored == want, (terms, int(word), stored)
