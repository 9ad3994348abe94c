"""-m gpu: the 96-features-per-wave form of gemm_ws_kernel (csrc/vit_gemm_ws.h, RT = 3: column groups of 384, three weight tiles per
wave, 72 MFMAs per step, the bias read from LDS in the slots) and the plan that lays its chunks out (gemm_ws96_plan, exported as
dtk_vit_gemm_ws_plan), against the untouched round 1-3 form of the kernel (DTK_VIT_GEMM_WS_V1).  Every output is the same chain of
24 MFMAs in both forms, so on the same operands every output BIT must agree.  Outputs start as a sentinel pattern (run_stage), so a
row that nobody wrote shows, and run_stage asserts every guard band.

fc1 (four column groups, equal chunks) and qkv (three groups: all-Q, all-K, all-V^T workgroups; Q / K staged as a workgroup-wide
tile and flushed as whole lines, V^T by 2-byte stores; the V^T group with more, shorter chunks) both run the new form.  Where the
library reports no plan (several frames shorter than a tile) the cases fall back to the layout of gemm_ws_grid.

Row counts: 1, 31, 32, 33, 64, 65, 113 and the smallest counts for which the launch's own layout gives 2, 3 and >= 5 tiles per chunk
with a short last chunk in every column group -- the peeled pair alone, the pair plus the odd tail, the steady state."""
import ctypes

import pytest
import torch

import vit_gemm_ref as R
from dino_tracker_amd._lib import lib
from test_gpu_vit_gemm import BF16, DEV, F16, WS_V1, run_stage
from test_gpu_vit_gemm_ws_epilogue import assert_same_bits, operands, sp_of

pytestmark = pytest.mark.gpu

D = 384
ROLES = {"qkv": R.QKV, "fc1": R.FC1}
WS96_COLS, WS96_WGS = 384, 256


def plan(role, rows, S=0, flags=0):
    """[(chunks, tiles per chunk, tiles of the last chunk)] per 384-column group as the library lays the launch out; [] when the role
    does not run the 96-feature form."""
    ch, tp, la = (ctypes.c_int * 4)(), (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
    g = lib().dtk_vit_gemm_ws_plan(role, D, flags, rows, S if S else rows, ch, tp, la)
    assert 0 <= g <= 4
    return [(ch[i], tp[i], la[i]) for i in range(g)]


def layout(role, rows, S=0):
    """(column-group width, [(chunks, tpc, last)] per group) of the default launch: the plan, or gemm_ws_grid (R.ws_grid)."""
    N, _ = R.shape(role, D)
    p = plan(role, rows, S)
    if p:
        assert len(p) * WS96_COLS == N
        return WS96_COLS, p
    return R.WS_COLS, [R.ws_grid(N, rows)] * (-(-N // R.WS_COLS))


def rows_for(role, lo, hi, step=1, unequal=False):
    """The smallest row count, a multiple of `step` with a ragged last tile, whose layout has in EVERY column group lo <= tiles per
    chunk <= hi, more than one chunk and a last chunk shorter than the others (unequal: and not the same tiles per chunk everywhere)."""
    for m in range(1, 1 << 20):
        rows = m * step
        _, groups = layout(role, rows, step if step > 1 else 0)
        if min(t for _, t, _ in groups) > hi:
            break
        ragged = rows % R.WS_ROWS == 17 if step == 1 else rows % R.WS_ROWS != 0
        if ragged and all(lo <= t <= hi and c > 1 and 0 < la < t for c, t, la in groups) and (not unequal or len({t for _, t, _ in groups}) > 1):
            return rows
    raise AssertionError((role, lo, hi, step))


def cases(role):
    """[(rows, S, Sp)]; S = 0 outside QKV."""
    if role != R.QKV:
        return [(r, 0, 0) for r in [1, 31, 32, 33, 64, 65, 113] + [rows_for(role, lo, hi) for lo, hi in ((2, 2), (3, 3), (5, 99))]]
    out = [(r, r, sp_of(r)) for r in (1, 31, 32, 33, 64, 65, 113)]
    out += [(7 * 21, 21, 64), (3 * 37, 37, 64), (3 * 222, 222, 256)]
    for s, lo, hi in ((37, 5, 99), (222, 2, 2), (222, 3, 3), (222, 5, 99)):
        out.append((rows_for(role, lo, hi, step=s), s, sp_of(s)))
    # the V^T group has chunks of its own: a count at which its tiles per chunk differ from the Q / K groups' and its last chunk is short
    rows = rows_for(role, 2, 99, step=222, unequal=True)
    _, groups = layout(role, rows, 222)
    assert groups[2][1] != groups[0][1] and groups[2][2] < groups[2][1], groups
    out.append((rows, 222, 256))
    return out


def test_plan_covers_every_tile_once():
    """No device memory: for N = 1152 (qkv) and N = 1536 (fc1) and a spread of row counts from 1 to 800 000, every token tile of every
    column group belongs to exactly one chunk, the chunks of a launch number at most 256, a chunk stays within 32-bit byte offsets,
    and launches with fewer tiles than chunks get one tile per chunk.  The plan is the documented one: fc1 four shares of 64 chunks,
    qkv (a, a, b) with b > a, 2 a + b <= 256, b a constant of the library (read off the benchmark shape's plan)."""
    counts = sorted({1, 31, 32, 33, 64, 65, 113, 2048, 2049, 2065, 4129, 8209, 8225, 16000, 65536, 100001, 729720, 799999, 800000}
                    | {r * 997 + 13 for r in range(1, 800, 37)})
    b = plan(R.QKV, 729720, 8108)[2][0]
    a = (WS96_WGS - b) // 2
    assert a < b and 2 * a + b <= WS96_WGS and plan(R.QKV, 729720, 8108)[0][0] == plan(R.QKV, 729720, 8108)[1][0] == a, (a, b)
    shares = {R.QKV: [a, a, b], R.FC1: [64] * 4}
    for role in (R.QKV, R.FC1):
        N, K = R.shape(role, D)
        assert plan(role, 729720, 8108, WS_V1) == [], "the A / B form runs on gemm_ws_grid"
        for rows in counts:
            p = plan(role, rows)
            tiles = -(-rows // R.WS_ROWS)
            assert len(p) == N // WS96_COLS and sum(c for c, _, _ in p) <= WS96_WGS, (role, rows, p)
            for (c, t, la), share in zip(p, shares[role]):
                assert c >= 1 and t >= 1 and 1 <= la <= t and (c - 1) * t + la == tiles, (role, rows, p)   # consecutive chunks: each tile once
                assert t * R.WS_ROWS * K * 2 < 2 ** 32
                if tiles <= share:
                    assert t == 1 and c == tiles
                assert t == max(1, -(-tiles // share)) and c == -(-tiles // t), (role, rows, p)
    assert plan(R.FC1, 729720) == [(64, 357, 313)] * 4   # the benchmark shape: 22804 tiles, four groups of 64 chunks, 256 workgroups
    assert plan(R.QKV, 7 * 21, 21) == [], "several frames shorter than a tile go to the tiled kernel"


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("role", list(ROLES))
def test_bitwise_against_v1(role, dt):
    """Flags 0 and DTK_VIT_GEMM_WS_V1 on the same operands: identical bits, the chunk shapes asserted against the launch's own layout."""
    dtype = F16 if dt == "fp16" else BF16
    r = ROLES[role]
    cs = cases(r)
    want_tpc = {2: 0, 3: 0, 5: 0}
    for i, (rows, S, Sp) in enumerate(cs):
        _, groups = layout(r, rows, S)
        for c, t, la in groups:
            assert (c - 1) * t + la == -(-rows // R.WS_ROWS)
        for k in want_tpc:
            want_tpc[k] += all((t == k if k < 5 else t >= 5) and 0 < la < t and c > 1 for c, t, la in groups)
        o = operands(r, dtype, rows, S, Sp, 9001 + 17 * i + 1000 * r + (dt == "bf16"))
        new, old = run_stage(o, 0), run_stage(o, WS_V1)
        assert_same_bits(new, old, f"{role} {dt} rows={rows} S={S}")
        if r == R.QKV:
            assert R.qkv_padding_is_zero(new["q"], new["k"], new["vt"], S), f"{role} {dt} rows={rows} S={S}: padding rows written"
    assert all(n >= 1 for n in want_tpc.values()), ("a chunk shape is missing from the cases", want_tpc)
    print(f"gemm_ws96 {role} {dt}: {len(cs)} row counts bit-equal to the V1 form")


def test_qkv_short_frames_go_to_the_tiled_kernel():
    """S = 21 x 7: several frames shorter than a tile.  The launcher sends them to the tiled kernel under either flag; both agree."""
    o = operands(R.QKV, F16, 7 * 21, 21, 64, 31)
    assert_same_bits(run_stage(o, 0), run_stage(o, WS_V1), "qkv S=21 x 7")


@pytest.mark.parametrize("role", list(ROLES))
def test_repeatable(role):
    """The >= 5-tile case three times into fresh outputs: equal bits."""
    r = ROLES[role]
    rows, S, Sp = [c for c in cases(r) if all(t >= 5 for _, t, _ in layout(r, c[0], c[1])[1])][0]
    o = operands(r, F16, rows, S, Sp, 1977 + r)
    first = run_stage(o, 0)
    for rep in (1, 2):
        assert_same_bits(run_stage(o, 0), first, f"{role} rows={rows} run {rep}")


@pytest.mark.parametrize("role", [R.QKV, R.FC1], ids=["qkv", "fc1"])
def test_overflow_word_in_steady_state(role):
    """GemmEpi::ovf through the slots of a steady-state step: one stored value of 65536 (256 products of 16 x 16) in the third tile of a
    chunk of >= 5 tiles, in the last column of EACH column group, sets bit 2 (QKV) / 4 (fc1) and is stored as the saturated 65504; 255
    products (65280) leave the word at 0."""
    N, K = R.shape(role, D)
    rows = rows_for(role, 5, 99)
    width, groups = layout(role, rows)
    assert all(t >= 5 for _, t, _ in groups)
    row = 2 * 32 + 5
    bit = 2 if role == R.QKV else 4
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    last_cols = [min(g * width + width, N) - 1 for g in range(len(groups))]
    assert last_cols[-1] == N - 1
    for col in last_cols:
        for terms, want_word, want in ((256, bit, 65504.0), (255, 0, 65280.0)):
            A, W = torch.zeros(rows, K, device=DEV), torch.zeros(N, K, device=DEV)
            A[row, :terms] = 16.0
            W[col, :256] = 16.0
            o = {"role": role, "D": D, "rows": rows, "dtype": F16, "split": False, "w_scale": 1.0, "exact": False, "S": rows, "Sp": sp_of(rows),
                 "A": A.to(F16), "W": W.to(F16), "bias": torch.zeros(N, device=DEV)}
            word.zero_()
            got = run_stage(o, 0, ovf=word)
            stored = float(R.matrix(o, got)[row, col])
            if role == R.QKV and col < D:
                want = float(torch.tensor(want * R.QSCALE, dtype=torch.float32).to(F16))   # Q carries log2(e) / 8: below the limit
                want_word = 0
            assert int(word) == want_word and stored == want, (col, terms, int(word), stored)
