"""CPU: the numpy restatement of docs/JPEG_DECODE.md (tests/jpeg_dec_ref.py) against Pillow's DECODER -- np.array_equal on whole
images --, its entropy stage against the encoder restatement's coefficients, the planted faults, the host-side header parser's
routing (dino_tracker_amd/video_in.py), and the stand-alone sanitiser build of the decode loop the kernel runs
(tests/host/jpeg_entropy_host.cpp).  The equality with Pillow holds for the Pillow / libjpeg-turbo builds docs/PARITY.md names."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_dec_cases as C
import jpeg_dec_ref as D
import jpeg_ref as J

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = sorted(set([(1, 1), (2, 16), (8, 16), (17, 9), (16, 16), (33, 50), (48, 160), (130, 23), (200, 40), (32, 854)] +
                   [(17, 17), (15, 33), (31, 47), (33, 70)]))
KINDS = ("noise", "ramp", "checker", "pm1")
QUALITIES = (5, 75, 90, 100)
HORSEJUMP = os.path.join(HERE, "golden", "horsejump_00000.jpg")


@pytest.fixture(scope="module")
def pillow():
    from PIL import features
    if not features.check("jpg"):
        pytest.skip("Pillow was built without a JPEG codec")
    return True


# ---- 1. the restatement equals Pillow's decoder; its entropy stage inverts the encoder's ------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_pillow(pillow, size):
    h, w = size
    for kind in KINDS:
        img = J.picture(kind, h, w)
        for q in QUALITIES:
            for name, data in C.variants(img, q):
                got = D.decode(data)          # exact=True: also asserts that no 32-bit operation wrapped
                assert got.shape == (h, w, 3)
                assert np.array_equal(got, C.pillow_decode(data)), (size, kind, q, name)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_coefficients_round_trip(size):
    h, w = size
    for kind in KINDS:
        img = J.picture(kind, h, w)
        for q in QUALITIES:
            want = J.coefficients(img, q)
            for R in (1, 3, 16):
                assert np.array_equal(D.coefficients(J.encode(img, q, R)), want), (size, kind, q, R)


def test_a_real_frame(pillow):
    """854 x 480, one scan of 3 240 MCUs without a restart marker, the encoder's own (optimised) Huffman tables"""
    with open(HORSEJUMP, "rb") as fh:
        data = fh.read()
    p = D.parse(data)
    assert (p["H"], p["W"], p["R"]) == (480, 854, 0)
    assert np.array_equal(D.decode(data), C.pillow_decode(data))


# ---- 2. planted faults -------------------------------------------------------------------------------------------------------------
def _fault_cases():
    """small files that between them reach every planted fault"""
    out = []
    # (4 x 16 and 20 x 24: an even height whose last chroma row is not the first of its block row -- the last pixel row looks DOWN,
    # and in the transform's padding stands a row that the quantisation made differ from the last real one)
    for (h, w), kind, q in (((17, 17), "noise", 90), ((15, 33), "noise", 75), ((4, 16), "noise", 75), ((20, 24), "noise", 75),
                            ((31, 47), "noise", 100),
                            ((33, 70), "checker", 90), ((33, 70), "noise", 5)):
        img = J.picture(kind, h, w)
        out += [(img, q, data) for _, data in C.variants(img, q)[1:3]]           # R = 3 and R = 16
    sparse = np.full((16, 16, 3), 128, np.uint8)
    sparse[::2, 1::2] = 131                                                        # the highest frequency alone: runs above 15
    out.append((sparse, 100, J.encode(sparse, 100, 16)))
    blue = np.zeros((16, 16, 3), np.uint8)
    blue[...] = (0, 0, 250)                                                        # Y = 28, Cb - 128 = 125: where 116130 +- 1 shows
    out.append((blue, 100, J.encode(blue, 100, 16)))
    return out


def test_every_fault_is_planted():
    import inspect
    src = inspect.getsource(D)
    for fault in D.FAULTS:
        assert src.count(f'"{fault}"') >= 2, fault     # in FAULTS and where it acts


@pytest.mark.parametrize("fault", D.FAULTS)
def test_planted_fault_is_noticed(pillow, fault):
    noticed = 0
    for img, q, data in _fault_cases():
        want_px, want_coef = C.pillow_decode(data), J.coefficients(img, q)
        try:
            coef = D.coefficients(data, faults=(fault,))
            px = D.decode(data, faults=(fault,), exact=False)
        except AssertionError:
            noticed += 1
            continue
        noticed += (not np.array_equal(coef, want_coef)) or (not np.array_equal(px, want_px))
    assert noticed >= 1, fault


# ---- 3. routing ------------------------------------------------------------------------------------------------------------------
def _save(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_eligible_files_and_their_segments(pillow):
    from dino_tracker_amd import video_in
    img = J.picture("noise", 33, 70)
    for name, data in C.variants(img, 90):
        h, why = video_in.parse_jpeg(data)
        assert h is not None, (name, why)
        p = D.parse(data)
        assert (h.height, h.width, h.restart) == (33, 70, p["R"]) and np.array_equal(h.qtables, p["qt"])
        for c in range(3):
            for cls in range(2):
                bits, vals = p["huff"][c][cls]
                assert h.huffman[c, cls].tobytes() == bytes(bits) + bytes(vals) + bytes(272 - 16 - len(vals))
        mcus, per = 15, h.restart or 15
        assert h.segments[:, 2].tolist() == list(range(0, mcus, per)) and int(h.segments[:, 3].sum()) == mcus
        # the segments are the scan without its markers
        scan = p["scan"]
        joined = b"".join(data[o:o + n] for o, n in h.segments[:, :2].tolist())
        assert len(joined) == len(scan) - 2 * (h.segments.shape[0] - 1) and data[h.scan[0]:h.scan[1]] == scan


def test_ineligible_files_name_their_reason(pillow):
    from dino_tracker_amd import video_in
    img = J.picture("noise", 33, 50)
    good = J.encode(img, 90, 3)
    assert video_in.parse_jpeg(good)[0] is not None
    adobe = good[:2] + b"\xff\xee\x00\x0e" + b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 1]) + good[2:]
    q16 = bytearray(good)
    at = good.index(b"\xff\xdb")
    wide = b"\xff\xdb" + (3 + 128).to_bytes(2, "big") + b"\x10" + b"".join(int(v).to_bytes(2, "big") for v in good[at + 5:at + 69])
    q16 = good[:at] + wide + good[at + 69:]
    first = good.index(b"\xff\xd0")
    swapped = bytearray(good)
    swapped[first + 1] = 0xD1
    for data, word in ((_save(img, progressive=True), "progressive"), (_save(img, subsampling=0), "4:4:4"),
                       (_save(img, subsampling=1), "4:2:2"), (_save(img[..., 0]), "grayscale"), (adobe, "Adobe"),
                       (q16, "16-bit quantisation"), (bytes(swapped), "out of order"),
                       (good[:first] + good[first + 2:], "restart markers"), (good[:40], "runs past the file"),
                       (b"\x89PNG" + good, "no SOI")):
        h, why = video_in.parse_jpeg(data)
        assert h is None and word in why, (word, why)
    plan, why = video_in.plan_jpeg([good, J.encode(J.picture("noise", 33, 66), 90)])
    assert plan is None and "file 1: 33 x 66, file 0 is 33 x 50" in why
    plan, why = video_in.plan_jpeg([good, good, _save(img, progressive=True)])
    assert plan is None and why.startswith("file 2: progressive")
    plan, why = video_in.plan_jpeg([good, J.encode(J.picture("ramp", 33, 50), 5, 16)])
    assert why is None and plan.frames == 2 and plan.segments[:, 0].tolist() == [0] * 4 + [1]
    assert int(plan.segments[4, 1]) == len(good) + C.scan_start(J.encode(J.picture("ramp", 33, 50), 5, 16))
    for bad_bits in ([0, 5] + [0] * 14, [2, 0, 1] + [0] * 13):        # over-subscribed lengths
        assert "over-subscribed" in video_in._check_huffman(0, bad_bits, bytes(sum(bad_bits)))
    assert "DC category" in video_in._check_huffman(0, [1] + [0] * 15, b"\x0c")
    assert "AC size" in video_in._check_huffman(1, [1] + [0] * 15, b"\x1b")


def test_damaged_files_reach_the_decoder():
    """the damaged files of jpeg_dec_cases keep a header the parser accepts: the device decoder is what has to notice them"""
    from dino_tracker_amd import video_in
    for name, data in C.damaged():
        h, why = video_in.parse_jpeg(data)
        assert h is not None and h.segments.shape[0] == 1, (name, why)


# ---- 4. the decode loop under the sanitisers -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler (CXX, g++, clang++) to build tests/host/jpeg_entropy_host.cpp")
    exe = str(tmp_path_factory.mktemp("host") / "jpeg_entropy_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-o", exe, os.path.join(HERE, "host", "jpeg_entropy_host.cpp")], check=True)
    return exe


def test_decode_loop_is_clean_under_the_sanitisers(host_program):
    done = subprocess.run([host_program], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.rstrip().endswith("ok"), done.stdout + done.stderr
    assert "393 streams" in done.stdout, done.stdout


def test_damaged_cases_pass_the_host_program(host_program, tmp_path):
    names, paths = [], []
    for name, data in [("good", C.good_file())] + C.damaged():
        path = tmp_path / f"{name}.case"
        path.write_bytes(C.case_file(data))
        names.append(name)
        paths.append(str(path))
    done = subprocess.run([host_program] + paths, capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    status = {name: int(line.split()[0]) for name, line in zip(names, done.stdout.splitlines())}
    assert status["good"] == 0 and status["flipped_bit"] != 0, status
    for name, want in C.STATUS.items():
        assert status[name] == want, status
