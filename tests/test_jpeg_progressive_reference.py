"""CPU: progressive (SOF2) JPEG files.  The restatement of docs/JPEG_DECODE.md "Progressive files" (tests/jpeg_prog_ref.py) against an
oracle that shares nothing with it -- the coefficients tests/jpeg_sampling_ref.py reads from the BASELINE file of the same picture and
settings, and Pillow's pixels of the progressive file --, its planted faults, the host-side parser, planner and level assignment
(dino_tracker_amd/video_in.py), and the stand-alone sanitiser build of the per-block routines the kernel runs
(tests/host/jpeg_progressive_host.cpp).  The equalities hold for the Pillow / libjpeg-turbo builds docs/PARITY.md names."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_prog_cases as C
import jpeg_prog_ref as P
import jpeg_sampling_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (3, 1), (5, 4), (4, 5), (9, 17), (17, 33), (31, 47), (33, 15), (40, 200)]
KINDS = ("noise", "ramp")
QUALITIES = (5, 75, 100)
COLOUR_LEVELS, GRAY_LEVELS = [0, 0, 0, 0, 0, 1, 1, 1, 1, 2], [0, 0, 0, 1, 1, 2]


@pytest.fixture(scope="module")
def pillow():
    from PIL import features
    if not features.check("jpg"):
        pytest.skip("Pillow was built without a JPEG codec")
    return True


# ---- 1. the restatement against the baseline oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_the_baseline_coefficients_and_pillow(pillow, size):
    h, w = size
    for sampling in C.SAMPLINGS:
        for kind in KINDS:
            for q in QUALITIES:
                for restart, _ in C.RESTARTS:
                    base, prog = C.pair(kind, h, w, sampling, q, restart)
                    what = (size, R.NAMES[sampling], kind, q, restart)
                    coef = P.coefficients(prog)
                    assert np.array_equal(coef, R.coefficients(base)), what
                    p = P.parse(prog)
                    assert (p["H"], p["W"], p["sampling"]) == (h, w, sampling), what
                    px = R.pixels(coef, p["qt"], h, w, sampling)
                    assert np.array_equal(px, C.pillow_decode(prog)) and np.array_equal(px, C.pillow_decode(base)), what


def test_a_real_frame(pillow):
    """854 x 480 re-encoded as a progressive file: ten scans without a restart marker, against Pillow's pixels and against the
    baseline file of the same pixels"""
    from PIL import Image
    prog = C.real_frame()
    p = P.parse(prog)
    assert (p["H"], p["W"], p["sampling"], len(p["scans"])) == (480, 854, R.S420, 10)
    with Image.open(C.HORSEJUMP) as img:
        base = C.encode(np.asarray(img.convert("RGB")), R.S420, 90, progressive=False)
    coef = P.coefficients(prog)
    assert np.array_equal(coef, R.coefficients(base))
    assert np.array_equal(R.pixels(coef, p["qt"], 480, 854, R.S420), C.pillow_decode(prog))


def test_long_end_of_band_runs(pillow):
    """a flat 1024 x 1024 picture with one differing pixel: runs of thousands of blocks, categories up to 14, in first and refinement
    scans (the small files reach 6)"""
    prog = C.flat_file()
    assert len(prog) < 6000
    info = {}
    coef = P.coefficients(prog, info=info)
    assert max(info["eob_categories"]["first"]) == 14 and max(info["eob_categories"]["refine"]) == 14, info
    img = np.full((1024, 1024), 128, np.uint8)
    img[517, 300] = 160
    assert np.array_equal(coef, R.coefficients(C.encode(img, R.GRAY, 75, progressive=False)))
    assert np.array_equal(R.pixels(coef, P.parse(prog)["qt"], 1024, 1024, R.GRAY), C.pillow_decode(prog))
    small = {}
    for sampling in C.SAMPLINGS:
        P.coefficients(C.pair("noise", 40, 200, sampling, 5)[1], info=small)
        assert max(small["eob_categories"]["first"] | small["eob_categories"]["refine"] | {0}) <= 8


# ---- 2. planted faults -------------------------------------------------------------------------------------------------------------------
def _fault_cases():
    """small files that between them reach every planted fault: 33 x 15 and 17 x 33 are where the real and the padded block grids of
    the subsampled layouts differ"""
    return [C.pair("noise", h, w, sampling, q, restart) for (h, w) in ((33, 15), (17, 33), (31, 47))
            for sampling in (R.S420, R.S422, R.GRAY) for q, restart in ((75, "none"), (100, "blocks3"))]


def test_every_fault_is_planted():
    import inspect
    src = inspect.getsource(P)
    assert len(P.FAULTS) >= 6
    for fault in P.FAULTS:
        assert src.count(f'"{fault}"') >= 2, fault     # in FAULTS and where it acts


@pytest.mark.parametrize("fault", P.FAULTS)
def test_planted_fault_is_noticed(pillow, fault):
    noticed = 0
    for base, prog in _fault_cases():
        want = R.coefficients(base)
        try:
            coef = P.coefficients(prog, faults=(fault,))
        except (AssertionError, IndexError):
            noticed += 1
            continue
        noticed += not np.array_equal(coef, want)
    assert noticed >= 1, fault


# ---- 3. the parser, the levels, the plan ---------------------------------------------------------------------------------------------------
def test_parser_accepts_pillows_files(pillow):
    from dino_tracker_amd import video_in
    for sampling in C.SAMPLINGS:
        for (h, w) in ((1, 1), (17, 33), (33, 15)):
            for restart, _ in C.RESTARTS:
                _, prog = C.pair("noise", h, w, sampling, 75, restart)
                hd, why = video_in.parse_jpeg_progressive(prog)
                assert hd is not None, (R.NAMES[sampling], h, w, restart, why)
                p = P.parse(prog)
                assert (hd.height, hd.width, hd.sampling) == (h, w, sampling) and np.array_equal(hd.qtables, p["qt"])
                assert video_in.scan_levels(hd.scans) == (GRAY_LEVELS if sampling == R.GRAY else COLOUR_LEVELS)
                assert len(hd.scans) == len(p["scans"])
                for scan, want in zip(hd.scans, p["scans"]):
                    assert (list(scan.components), scan.ss, scan.se, scan.ah, scan.al) == (want["comps"], want["Ss"], want["Se"],
                                                                                          want["Ah"], want["Al"])
                    assert scan.restart == want["R"]
                    units = video_in.scan_units(h, w, sampling, scan.components)
                    rows, cols = P.component_grid(h, w, sampling, scan.components[0])
                    assert units == (np.prod(R.mcu_grid(h, w, sampling)) if len(scan.components) > 1 else rows * cols)
                    per = scan.restart or units
                    assert scan.segments[:, 2].tolist() == list(range(0, units, per)) and int(scan.segments[:, 3].sum()) == units
                    # the segments are the body without its markers
                    joined = b"".join(prog[o:o + n] for o, n in scan.segments[:, :2].tolist())
                    assert len(joined) == len(want["body"]) - 2 * (scan.segments.shape[0] - 1)
                    # the tables are the ones in force at the SOS
                    if scan.ss == 0 and scan.ah == 0:
                        raws = [want["huff"][c][0] for c in range(len(want["comps"]))]
                    else:
                        raws = [want["huff"][0][1]] if scan.ss else []
                    assert [t for t in scan.tables] == [bytes(b) + bytes(v) + bytes(272 - 16 - len(v)) for b, v in raws]


def test_ineligible_files_name_their_reason(pillow):
    from dino_tracker_amd import video_in
    base, prog = C.pair("noise", 33, 50, R.S420, 90)
    assert video_in.parse_jpeg_progressive(prog)[0] is not None
    p444 = C.pair("noise", 33, 50, R.S444, 90)[1]
    for data, word in ((C.cut_after_scans(prog, 5), "incomplete progression"),
                       (C.with_scan_bits(prog, 5, 1, 1), "not the successor"),        # luma 1-63 refinement: 2/1 -> 1/1
                       (C.with_scan_bits(prog, 1, 1, 0), "not the successor"),        # a band's first scan with Ah = 1 ...
                       (C.with_scan_bits(prog, 6, 0, 0), "coded already"),             # ... and a second "first" scan of DC
                       (C.dqt_behind_first_scan(prog), "DQT behind the first SOS"),
                       (base, "not progressive"),
                       (C.sof_factors_patched(p444, 0x12), "4:4:0"),
                       (prog[:len(prog) // 2], "file ends inside the scan"),
                       (b"\x89PNG" + prog, "no SOI")):
        hd, why = video_in.parse_jpeg_progressive(data)
        assert hd is None and word in why, (word, why)
    plan, why = video_in.plan_jpeg_progressive([prog, C.pair("noise", 33, 66, R.S420, 90)[1]])
    assert plan is None and "file 1: 33 x 66, file 0 is 33 x 50" in why
    plan, why = video_in.plan_jpeg_progressive([prog, p444])
    assert plan is None and "file 1: sampling 4:4:4, file 0 is 4:2:0" in why
    plan, why = video_in.plan_jpeg_progressive([prog, prog, base])
    assert plan is None and why.startswith("file 2: not progressive")


def test_the_old_functions_still_refuse_progressive_files(pillow):
    from dino_tracker_amd import video_in
    _, prog = C.pair("noise", 33, 50, R.S420, 90)
    assert video_in.parse_jpeg(prog) == (None, "progressive (SOF2)")
    assert video_in.parse_jpeg_sampled(prog) == (None, "progressive (SOF2)")
    assert video_in.plan_jpeg([prog]) == (None, "file 0: progressive (SOF2)")
    assert video_in.plan_jpeg_sampled([prog]) == (None, "file 0: progressive (SOF2)")
    assert video_in._SOF_OTHERS[0xC2] == "progressive (SOF2)"


def test_scan_levels():
    from dino_tracker_amd.video_in import JpegScan, scan_levels

    def scan(components, ss, se, ah=0, al=0):
        return JpegScan(tuple(components), ss, se, ah, al, (), 0, np.zeros((0, 4), np.int64))
    colour = [scan((0, 1, 2), 0, 0, 0, 1), scan((0,), 1, 5, 0, 2), scan((2,), 1, 63, 0, 1), scan((1,), 1, 63, 0, 1), scan((0,), 6, 63, 0, 2),
              scan((0,), 1, 63, 2, 1), scan((0, 1, 2), 0, 0, 1, 0), scan((2,), 1, 63, 1, 0), scan((1,), 1, 63, 1, 0), scan((0,), 1, 63, 1, 0)]
    assert scan_levels(colour) == COLOUR_LEVELS
    gray = [scan((0,), 0, 0, 0, 1), scan((0,), 1, 5, 0, 2), scan((0,), 6, 63, 0, 2), scan((0,), 1, 63, 2, 1), scan((0,), 0, 0, 1, 0),
            scan((0,), 1, 63, 1, 0)]
    assert scan_levels(gray) == GRAY_LEVELS
    # bands that overlap only partly are ordered all the same; another component's are not
    assert scan_levels([scan((0,), 1, 5), scan((0,), 3, 63), scan((1,), 3, 63), scan((0,), 6, 63), scan((0,), 0, 0)]) == [0, 1, 0, 2, 0]
    assert scan_levels([]) == []


def test_plan_orders_rows_by_level_and_shares_tables(pillow):
    from dino_tracker_amd import video_in
    files = [C.pair("noise", 17, 33, R.S420, 90, "blocks3")[1], C.pair("ramp", 17, 33, R.S420, 75)[1],
             C.pair("noise", 17, 33, R.S420, 90, "blocks3")[1]]
    offsets = np.concatenate(([0], np.cumsum([len(f) for f in files])))
    plan, why = video_in.plan_jpeg_progressive(files)
    assert why is None and plan.frames == 3 and plan.segments.shape[1] == 14 and plan.qtables.shape == (3, 3, 64)
    rows = plan.segments
    assert (np.diff(rows[:, 3]) >= 0).all() and set(rows[:, 3].tolist()) == {0, 1, 2}
    for f in range(3):
        mine = rows[rows[:, 0] == f]
        assert ((mine[:, 1] >= offsets[f]) & (mine[:, 1] + mine[:, 2] <= offsets[f + 1])).all()
    same = rows[rows[:, 0] == 0].copy(), rows[rows[:, 0] == 2].copy()
    same[1][:, 0], same[1][:, 1] = 0, same[1][:, 1] - offsets[2]
    assert np.array_equal(same[0], same[1])                      # the same file twice: the same rows, the same (shared) tables
    assert plan.tables.shape[0] < 2 * 10 + 10                    # at most ten distinct tables per distinct file


# ---- 4. the per-block routines under the sanitisers ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler (CXX, g++, clang++) to build tests/host/jpeg_progressive_host.cpp")
    exe = str(tmp_path_factory.mktemp("host") / "jpeg_progressive_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-o", exe, os.path.join(HERE, "host", "jpeg_progressive_host.cpp")], check=True)
    return exe


def test_built_in_streams_are_clean_under_the_sanitisers(host_program):
    done = subprocess.run([host_program], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.rstrip().endswith("ok"), done.stdout + done.stderr
    assert "106 streams" in done.stdout, done.stdout


def test_pillows_files_pass_the_host_program(pillow, host_program, tmp_path):
    """valid segments of all four scan kinds from exact-size buffers, and a few hundred damaged ones per file"""
    files = [C.pair("noise", 33, 15, R.S420, 75)[1], C.pair("noise", 17, 33, R.S420, 75, "blocks3")[1],
             C.pair("noise", 17, 33, R.S422, 100, "rows1")[1], C.pair("noise", 40, 200, R.GRAY, 75)[1],
             C.pair("noise", 31, 47, R.S444, 75, "blocks3")[1], C.flat_file(), C.real_frame()]
    paths = []
    for n, data in enumerate(files):
        path = tmp_path / f"{n}.case"
        path.write_bytes(C.case_file(data))
        paths.append(str(path))
    done = subprocess.run([host_program] + paths, capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.rstrip().endswith("ok"), done.stdout + done.stderr
    lines = done.stdout.splitlines()
    assert len(lines) == 9 and all("4 scan kinds damaged" in line for line in lines[:7]), done.stdout
    assert int(lines[7].split()[0]) > 2000, done.stdout
