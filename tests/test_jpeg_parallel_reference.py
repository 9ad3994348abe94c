"""CPU: decoding inside a JPEG segment with sub-streams (docs/JPEG_DECODE.md section 1b).  The plain-Python restatement
tests/jpeg_par_ref.py must give the coefficients of the sequential restatement tests/jpeg_sampling_ref.py -- which the other CPU
files hold to Pillow -- on the files of tests/jpeg_sampling_cases.py and tests/jpeg_dec_cases.py, for sub-streams of 16, 64 and 128
bytes; on a flat picture (hundreds of blocks start in one sub-stream) and on quality-100 noise (blocks longer than a sub-stream,
guesses that hardly ever merge: the case that rests on the fixpoint alone); planted faults are each noticed.  The stand-alone program
tests/host/jpeg_parallel_host.cpp runs the header's own functions under the sanitisers."""
import os
import shutil
import statistics
import subprocess

import numpy as np
import pytest

import jpeg_dec_cases as C
import jpeg_par_ref as P
import jpeg_ref as J
import jpeg_sampling_cases as SC
import jpeg_sampling_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "horsejump_00000.jpg")
SIZES = [(1, 1), (5, 4), (9, 17), (17, 33), (31, 47), (40, 200)]
LENGTHS = (16, 64, 128)
name_of = R.NAMES.get


def merged(info):
    """the guesses' merge distances of one segment, None (never) left out"""
    return sorted(d for d in info["distances"] if d is not None)


@pytest.mark.parametrize("sampling", SC.SAMPLINGS, ids=name_of)
def test_substreams_give_the_sequential_coefficients(sampling):
    files = 0
    for h, w in SIZES:
        for quality in ((75, 100) if (h, w) == (17, 33) else (75,)):
            for name, data in SC.variants(SC.picture("noise", h, w, sampling), sampling, quality):
                want = R.coefficients(data)
                for L in LENGTHS:
                    assert np.array_equal(P.coefficients(data, L), want), (h, w, quality, name, L)
                files += 1
    assert files == (len(SIZES) + 1) * 4


def test_the_first_decoder_s_stream_variants():
    """4:2:0 through the encoder restatement at restart intervals 1, 3 and 16 and Pillow's four variants"""
    for h, w in ((9, 17), (31, 47), (40, 200)):
        for name, data in C.variants(J.picture("noise", h, w), 90):
            want = R.coefficients(data)
            for L in LENGTHS:
                assert np.array_equal(P.coefficients(data, L), want), (h, w, name, L)


# what the real frame's one segment (66 290 scan bytes, 9 720 blocks) takes: docs/JPEG_DECODE.md section 1b quotes these
GOLDEN_RECORD = {128: dict(substreams=518, rounds=10, median=0.54, p99=4.83, longest=8.56),
                 64: dict(substreams=1036, rounds=20, median=1.08, p99=10.66, longest=18.12)}


@pytest.mark.parametrize("L", sorted(GOLDEN_RECORD))
def test_the_real_frame(L):
    data = open(GOLDEN, "rb").read()
    info = []
    assert np.array_equal(P.coefficients(data, L, info=info, distances=True), R.coefficients(data))
    assert len(info) == 1                                   # no restart markers: one segment
    d, want = merged(info[0]), GOLDEN_RECORD[L]
    assert len(d) == info[0]["substreams"] - 1, "with recovery every guess merges"
    got = dict(substreams=info[0]["substreams"], rounds=info[0]["rounds"], median=round(statistics.median(d), 2),
               p99=round(d[int(0.99 * len(d))], 2), longest=round(d[-1], 2))
    assert got == want
    # synchronous rounds: a state is final one round after its predecessor's, so the rounds follow the longest merge distance
    assert got["rounds"] <= int(d[-1]) + 3


def test_a_flat_picture_merges_at_once():
    """256 x 256 of one colour: 1 536 blocks of a few bits each, well over a hundred of them start in every 128-byte sub-stream"""
    for sampling, blocks in ((R.S420, 1536), (R.GRAY, 1024)):
        img = np.full((256, 256, 3), 90, dtype=np.uint8) if sampling != R.GRAY else np.full((256, 256), 90, dtype=np.uint8)
        data = SC.encode(img, sampling, 75)
        info = []
        coef = P.coefficients(data, 128, info=info, distances=True)
        assert np.array_equal(coef, R.coefficients(data)) and coef.shape[0] * coef.shape[1] == blocks
        assert info[0]["substreams"] >= 2 and blocks / info[0]["substreams"] > 100
        if sampling == R.S420:
            # (the last guess stands in the segment's last bits and reaches the end before it merges; in the gray file, whose blocks
            # are all the same six bits, a guess out of phase never merges at all: the fixpoint does not need it to)
            assert all(x is not None for x in info[0]["distances"][:-1]) and max(merged(info[0])) < 1.0


def noise_100(h=64, w=64, sampling=R.S420):
    return SC.encode(SC.picture("noise", h, w, sampling), sampling, 100)


def test_noise_at_quality_100_rests_on_the_fixpoint():
    """blocks longer than a sub-stream, and most guesses do not merge within two sub-streams: the result is right all the same"""
    data = noise_100()
    want = R.coefficients(data)
    for L in (16, 64, 128):
        info = []
        assert np.array_equal(P.coefficients(data, L, info=info, distances=True), want), L
        seg = info[0]
        assert len(info) == 1 and seg["longest_block_bits"] == 758
        if L < 128:                                         # (758 bits are 95 bytes: at 128 a block still spans two sub-streams at most)
            assert seg["longest_block_bits"] > 8 * L
        far = sum(1 for d in seg["distances"] if d is None or d > 2.0)
        assert far > len(seg["distances"]) / 2, (L, far, len(seg["distances"]))
        assert seg["rounds"] > seg["substreams"] // 2       # here the method degrades towards sequential


def dc_wrap_file():
    """a gray 8 x 160 file whose 20 blocks each code the DC difference +2047 and nothing else: the predictor passes 32 767"""
    data = SC.encode(SC.picture("noise", 8, 160, R.GRAY), R.GRAY, 75)
    (dc_bits, dc_vals), (ac_bits, ac_vals) = R.parse(data)["huff"][0]

    def code_of(bits, vals, symbol):
        code, k = 0, 0
        for n in range(1, 17):
            for _ in range(bits[n - 1]):
                if vals[k] == symbol:
                    return format(code, f"0{n}b")
                code, k = code + 1, k + 1
            code <<= 1
        raise AssertionError(symbol)

    text = (code_of(dc_bits, dc_vals, 11) + "1" * 11 + code_of(ac_bits, ac_vals, 0)) * 20   # category 11, the 11 bits of 2047, EOB
    text += "1" * (-len(text) % 8)
    scan = bytes(int(text[i:i + 8], 2) for i in range(0, len(text), 8)).replace(b"\xff", b"\xff\x00")
    return data[:C.scan_start(data)] + scan + b"\xff\xd9"


def test_dc_sums_wrap_to_int16():
    data = dc_wrap_file()
    want = R.coefficients(data)
    assert want[-1, 0, 0] == np.int16(20 * 2047 - 65536) and want[15, 0, 0] == 16 * 2047
    for L in LENGTHS:
        assert np.array_equal(P.coefficients(data, L), want)


FAULT_INPUTS = {"equal_by_position": lambda: SC.encode(SC.picture("noise", 40, 200, R.S420), R.S420, 75),
                "two_rounds": noise_100,
                "dc_saturates": dc_wrap_file,
                "count_block_ends": lambda: SC.encode(SC.picture("noise", 17, 33, R.S444), R.S444, 75)}


@pytest.mark.parametrize("fault", P.FAULTS)
def test_planted_faults_are_noticed(fault):
    data = FAULT_INPUTS[fault]()
    want = R.coefficients(data)
    assert np.array_equal(P.coefficients(data, 16), want)
    try:
        got = P.coefficients(data, 16, faults=(fault,))
    except (P.Invalid, AssertionError, IndexError):
        return                                              # the strict pass fell over: noticed
    assert not np.array_equal(got, want), fault


def test_every_fault_has_an_input():
    assert set(FAULT_INPUTS) == set(P.FAULTS)


# ---- the header's own functions under the sanitisers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler (CXX, g++, clang++) to build tests/host/jpeg_parallel_host.cpp")
    exe = str(tmp_path_factory.mktemp("host") / "jpeg_parallel_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-o", exe, os.path.join(HERE, "host", "jpeg_parallel_host.cpp")], check=True)
    return exe


def test_substream_functions_are_clean_under_the_sanitisers(host_program):
    done = subprocess.run([host_program], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.rstrip().endswith("ok") and "streams" in done.stdout, done.stdout
