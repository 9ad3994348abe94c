"""CPU: the numpy restatement of docs/JPEG_DECODE.md for every sampling (tests/jpeg_sampling_ref.py) against Pillow's DECODER --
np.array_equal on whole images --, its planted faults, the wide header parser and planner (video_in.parse_jpeg_sampled /
plan_jpeg_sampled) beside the narrow ones, and the stand-alone sanitiser build of the MCU schedule and decode loop the kernel runs
(tests/host/jpeg_entropy_sampled_host.cpp).  The equality with Pillow holds for the Pillow / libjpeg-turbo builds docs/PARITY.md
names."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_dec_cases as C
import jpeg_dec_ref as D
import jpeg_ref as J
import jpeg_sampling_cases as SC
import jpeg_sampling_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
# H x W: chroma planes 1, 2 and 3 samples wide, partial last MCUs both ways, a single block row
SIZES = [(1, 1), (1, 2), (3, 1), (2, 3), (5, 4), (4, 5), (7, 6), (8, 8), (9, 17), (16, 16), (17, 33), (31, 47), (33, 15), (24, 5),
         (40, 200)]
KINDS = ("noise", "ramp")
QUALITIES = (5, 75, 100)


@pytest.fixture(scope="module")
def pillow():
    from PIL import features
    if not features.check("jpg"):
        pytest.skip("Pillow was built without a JPEG codec")
    return True


# ---- 1. the restatement equals Pillow's decoder ------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sampling", SC.SAMPLINGS, ids=lambda s: R.NAMES[s])
def test_restatement_equals_pillow(pillow, sampling, size):
    h, w = size
    for kind in KINDS:
        img = SC.picture(kind, h, w, sampling)
        for q in QUALITIES:
            for name, data in SC.variants(img, sampling, q):
                p = R.parse(data)
                assert (p["H"], p["W"], p["sampling"]) == (h, w, sampling), (size, kind, q, name)
                got = R.decode(data)          # exact=True: also asserts that no 32-bit operation wrapped
                assert got.shape == ((h, w) if sampling == R.GRAY else (h, w, 3))
                assert np.array_equal(got, SC.pillow_decode(data)), (R.NAMES[sampling], size, kind, q, name)


def test_restatements_agree_where_the_old_one_is_right(pillow):
    """4:2:0 with a chroma plane more than two samples wide: tests/jpeg_dec_ref.py is this restatement; narrower, it is not Pillow"""
    for (h, w), same in (((17, 33), True), ((5, 5), True), ((5, 4), False), ((3, 1), False)):
        data = SC.encode(SC.picture("noise", h, w, R.S420), R.S420, 75)
        assert np.array_equal(R.coefficients(data), D.coefficients(data))
        assert np.array_equal(R.decode(data), D.decode(data)) == same, (h, w)


def test_adobe_and_gray_factors_do_not_change_the_pixels(pillow):
    for sampling in (R.S444, R.S422, R.S420):
        data = SC.encode(SC.picture("noise", 17, 33, sampling), sampling, 75)
        for keep_jfif in (True, False):
            adobe = SC.with_adobe(data, 1, keep_jfif)
            assert R.parse(adobe)["adobe"] == 1
            assert np.array_equal(R.decode(adobe), SC.pillow_decode(adobe)) and np.array_equal(R.decode(adobe), R.decode(data))
    gray = SC.encode(SC.picture("noise", 17, 33, R.GRAY), R.GRAY, 75)
    for factors in (0x22, 0x21, 0x12):
        patched = SC.gray_with_factors(gray, factors)
        assert R.parse(patched)["factors"] == (factors,)
        assert np.array_equal(R.decode(patched), SC.pillow_decode(patched)) and np.array_equal(R.decode(patched), R.decode(gray))


# ---- 2. planted faults -------------------------------------------------------------------------------------------------------------
def _fault_cases():
    """small files that between them reach every planted fault: both narrow planes, both edges, a 2 x 2 SOF on a gray file"""
    out = []
    for sampling, (h, w), kind, q in ((R.S422, (9, 17), "noise", 75), (R.S422, (5, 4), "noise", 100), (R.S422, (3, 3), "noise", 100),
                                      (R.S420, (5, 4), "noise", 100), (R.S420, (4, 2), "noise", 100), (R.S422, (16, 32), "ramp", 75)):
        out.append(SC.encode(SC.picture(kind, h, w, sampling), sampling, q))
    for h, w in ((16, 32), (17, 33)):
        out.append(SC.gray_with_factors(SC.encode(SC.picture("noise", h, w, R.GRAY), R.GRAY, 90), 0x22))
    return out


def test_every_fault_is_planted():
    import inspect
    src = inspect.getsource(R)
    for fault in R.FAULTS:
        assert src.count(f'"{fault}"') >= 2, fault     # in FAULTS and where it acts


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_is_noticed(pillow, fault):
    noticed = 0
    for data in _fault_cases():
        want = SC.pillow_decode(data)
        assert np.array_equal(R.decode(data), want)
        try:
            got = R.decode(data, faults=(fault,), exact=False)
        except AssertionError:
            noticed += 1
            continue
        noticed += not np.array_equal(got, want)
    assert noticed >= 1, fault


# ---- 3. the parsers ----------------------------------------------------------------------------------------------------------------
def _files(h=33, w=50, q=90):
    return {s: SC.encode(SC.picture("noise", h, w, s), s, q, restart_marker_blocks=3) for s in SC.SAMPLINGS}


def test_wide_parser_accepts_the_four_samplings(pillow):
    from dino_tracker_amd import video_in
    assert (video_in.GRAY, video_in.S444, video_in.S422, video_in.S420) == (R.GRAY, R.S444, R.S422, R.S420)
    for sampling, data in _files().items():
        h, why = video_in.parse_jpeg_sampled(data)
        assert h is not None, (R.NAMES[sampling], why)
        p = R.parse(data)
        ncomp = 1 if sampling == R.GRAY else 3
        mh, mw = R.mcu_grid(33, 50, sampling)
        assert (h.height, h.width, h.sampling, h.restart, h.adobe) == (33, 50, sampling, 3, False) and h.mcus == mh * mw
        assert h.qtables.shape == (ncomp, 64) and np.array_equal(h.qtables, p["qt"]) and h.huffman.shape == (ncomp, 2, 272)
        for c in range(ncomp):
            for cls in range(2):
                bits, vals = p["huff"][c][cls]
                assert h.huffman[c, cls].tobytes() == bytes(bits) + bytes(vals) + bytes(272 - 16 - len(vals))
        assert h.segments[:, 2].tolist() == list(range(0, h.mcus, 3)) and int(h.segments[:, 3].sum()) == h.mcus
        joined = b"".join(data[o:o + n] for o, n in h.segments[:, :2].tolist())
        assert len(joined) == len(p["scan"]) - 2 * (h.segments.shape[0] - 1) and data[h.scan[0]:h.scan[1]] == p["scan"]
    gray = SC.gray_with_factors(_files()[R.GRAY], 0x22)
    h, why = video_in.parse_jpeg_sampled(gray)
    assert h is not None and h.sampling == R.GRAY and h.mcus == 5 * 7, why


def test_wide_parser_and_adobe(pillow):
    from dino_tracker_amd import video_in
    files = _files()
    for sampling in (R.S444, R.S422, R.S420):
        for keep_jfif in (True, False):
            h, why = video_in.parse_jpeg_sampled(SC.with_adobe(files[sampling], 1, keep_jfif))
            assert h is not None and h.adobe and h.sampling == sampling, why
        for transform in (0, 2):
            h, why = video_in.parse_jpeg_sampled(SC.with_adobe(files[sampling], transform))
            assert h is None and "Adobe" in why and f"transform {transform}" in why, why
    h, why = video_in.parse_jpeg_sampled(SC.with_adobe(files[R.GRAY], 1))
    assert h is None and "Adobe" in why and "1 component" in why, why


def test_wide_parser_refusals_and_the_planner(pillow):
    from dino_tracker_amd import video_in
    files = _files()
    img = SC.picture("noise", 33, 50, R.S444)
    h, why = video_in.parse_jpeg_sampled(SC.sof_factors_patched(files[R.S444], 0x12))
    assert h is None and "4:4:0" in why, why
    h, why = video_in.parse_jpeg_sampled(SC.sof_factors_patched(files[R.S444], 0x41))
    assert h is None and "4:1:1" in why, why
    h, why = video_in.parse_jpeg_sampled(SC.encode(img, R.S444, 90, progressive=True))
    assert h is None and "progressive" in why, why
    for sampling, data in files.items():
        plan, why = video_in.plan_jpeg_sampled([data, data])
        ncomp = 1 if sampling == R.GRAY else 3
        assert why is None and (plan.frames, plan.height, plan.width, plan.sampling) == (2, 33, 50, sampling)
        assert plan.huffman.shape == (2, ncomp, 2, 272) and plan.qtables.shape == (2, ncomp, 64)
        assert int(plan.segments[plan.segments[:, 0] == 1][0, 1]) == len(data) + C.scan_start(data)
    plan, why = video_in.plan_jpeg_sampled([files[R.S444], files[R.S420]])
    assert plan is None and why == "file 1: sampling 4:2:0, file 0 is 4:4:4"
    plan, why = video_in.plan_jpeg_sampled([files[R.GRAY], files[R.S422]])
    assert plan is None and why == "file 1: sampling 4:2:2, file 0 is grayscale"
    plan, why = video_in.plan_jpeg_sampled([files[R.S422], SC.encode(SC.picture("noise", 33, 66, R.S422), R.S422, 90)])
    assert plan is None and "file 1: 33 x 66, file 0 is 33 x 50" in why
    plan, why = video_in.plan_jpeg_sampled([files[R.S444], SC.encode(img, R.S444, 90, progressive=True)])
    assert plan is None and why.startswith("file 1: progressive")


def test_narrow_parser_refuses_what_it_refused(pillow):
    """parse_jpeg / plan_jpeg are for 4:2:0 without an Adobe segment, with the words they always used"""
    from dino_tracker_amd import video_in
    files = _files()
    for data, why_want in ((files[R.S444], "sampling 4:4:4, not 4:2:0"), (files[R.S422], "sampling 4:2:2, not 4:2:0"),
                           (files[R.GRAY], "grayscale (1 component)"), (SC.with_adobe(files[R.S420]), "Adobe APP14 segment"),
                           (SC.with_adobe(files[R.S444]), "Adobe APP14 segment")):
        h, why = video_in.parse_jpeg(data)
        assert h is None and why == why_want, why
        plan, why = video_in.plan_jpeg([files[R.S420], data])
        assert plan is None and why == f"file 1: {why_want}"
    h, why = video_in.parse_jpeg(files[R.S420])
    assert why is None and h.sampling == R.S420 and not h.adobe
    plan, why = video_in.plan_jpeg([files[R.S420]])
    assert why is None and plan.sampling == R.S420


# ---- 4. the schedule and the decode loop under the sanitisers ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler (CXX, g++, clang++) to build tests/host/jpeg_entropy_sampled_host.cpp")
    exe = str(tmp_path_factory.mktemp("host") / "jpeg_entropy_sampled_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-o", exe, os.path.join(HERE, "host", "jpeg_entropy_sampled_host.cpp")], check=True)
    return exe


def test_schedules_are_clean_under_the_sanitisers(host_program):
    done = subprocess.run([host_program], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.rstrip().endswith("ok"), done.stdout + done.stderr
    assert "796 streams" in done.stdout, done.stdout          # 4 samplings x (1 + 64 + 1 + 128 + 4 + 1)
