"""CPU: the numpy restatement of docs/JPEG.md (tests/jpeg_ref.py) against Pillow's encoder, byte for byte; the host half of
dino_tracker_amd/video_out.py (tables, header, the AVI container) against Pillow's files and against its own strict reader.

The restatement is what tests/test_gpu_jpeg.py holds the device encoder to, so this file is what ties the device's bytes to an
encoder the world uses.  The comparison is of WHOLE FILES (Pillow writes the same header segments in the same order); where a
machine's Pillow cannot encode JPEG or does not know `restart_marker_blocks` the Pillow tests skip and say so, but never where
`features.check("jpg")` is true and the keyword is accepted -- which includes the machine this was built on."""
import io
import os
import struct

import numpy as np
import pytest

import jpeg_ref as J
from dino_tracker_amd import video_out as V

SIZES = [(1, 1), (2, 16), (8, 16), (17, 9), (16, 16), (33, 50), (48, 160), (130, 23), (200, 40), (32, 854)]
QUALITIES = (5, 75, 90, 100)
RESTARTS = (1, 3, 16)
CONTENTS = (("noise", QUALITIES), ("ramp", QUALITIES), ("checker", QUALITIES), ("pm1", (10,)))


def pillow_jpeg(img, q, R):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling=2, restart_marker_blocks=R)
    return buf.getvalue()


@pytest.fixture(scope="module")
def pillow():
    """skips when this Pillow cannot be the yardstick -- and refuses to skip when its JPEG codec is there"""
    from PIL import features
    if not features.check("jpg"):
        pytest.skip("Pillow was built without a JPEG codec")
    try:
        data = pillow_jpeg(np.zeros((16, 32, 3), np.uint8), 90, 1)
        segs, _ = J.split(data)
        dri = [p for m, p in segs if m == 0xDD]
        assert dri and int.from_bytes(dri[0], "big") == 1, "restart_marker_blocks was ignored"
    except Exception as e:   # noqa: BLE001
        raise AssertionError(f"Pillow has a JPEG codec but cannot write the comparison files: {e!r}")
    return True


def cases():
    for h, w in SIZES:
        for kind, qualities in CONTENTS:
            for q in qualities:
                for R in RESTARTS:
                    yield h, w, kind, q, R


# ---- 1. byte equality with Pillow ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_files_equal_pillows(pillow, size):
    h, w = size
    n = 0
    for kind, qualities in CONTENTS:
        img = J.picture(kind, h, w)
        for q in qualities:
            coef = J.coefficients(img, q)
            for R in RESTARTS:
                mine = J.header(h, w, q, R) + J.scan(coef, R) + b"\xff\xd9"
                theirs = pillow_jpeg(img, q, R)
                assert J.split(mine)[1] == J.split(theirs)[1], f"scan differs: {h} x {w} {kind} q{q} R{R}"
                assert mine == theirs, f"header differs: {h} x {w} {kind} q{q} R{R}"
                n += 1
    assert n == 39


def test_the_pictures_reach_the_corners_of_the_coder():
    """what the contents are there for: category-11 DC differences and EOB-only blocks (checker), runs of 16 and more zeros
    between coefficients, so ZRL (noise at quality 5), blocks whose 64th coefficient is coded (noise at quality 100), stuffed bytes.
    The +-1 noise around 128 at quality 10 quantises to nothing at all: it is the all-zero picture with every DC difference 0."""
    c = J.coefficients(J.picture("checker", 48, 160), 100).astype(np.int64)
    y = c[:, :4, 0].reshape(-1)
    assert np.abs(np.diff(y)).max() >= 1024 and (c[:, :, 1:] == 0).all()
    assert not J.coefficients(J.picture("pm1", 48, 160), 10).any()
    z = J.coefficients(J.picture("noise", 48, 160), 5).astype(np.int64)
    runs = [np.diff(np.flatnonzero(np.r_[1, b[1:]])).max(initial=0) for b in z.reshape(-1, 64)]
    assert max(runs) > 16
    assert (J.coefficients(J.picture("noise", 48, 160), 100)[:, :, 63] != 0).any()
    assert b"\xff\x00" in J.scan(J.coefficients(J.picture("noise", 48, 160), 100))


# ---- 2. tables -------------------------------------------------------------------------------------------------------------------
def test_tables_equal_pillows(pillow):
    img = J.picture("ramp", 16, 16)
    for q in range(1, 101):
        dqt, dht = J.tables_of(pillow_jpeg(img, q, 16))
        mine = V.quant_tables(q)
        assert mine.dtype == np.uint8 and mine.shape == (2, 64)
        assert dqt[0] == mine[0].tolist() and dqt[1] == mine[1].tolist(), q
        assert (np.stack(J.quant_tables(q)) == mine).all()
    _, ours = J.tables_of(V.jpeg_header(16, 16, 90) + b"\xff\xd9")
    assert sorted(ours) == [0x00, 0x01, 0x10, 0x11] and ours == dht
    assert ours == {i: (list(t[0]), list(t[1])) for i, t in
                    ((0x00, J.DC_LUMA), (0x10, J.AC_LUMA), (0x01, J.DC_CHROMA), (0x11, J.AC_CHROMA))}
    for bad in (0, 101, 50.5):
        with pytest.raises(ValueError):
            V.quant_tables(bad)


def test_header_equals_pillows_and_the_restatements(pillow):
    for (h, w), q in zip(SIZES, (5, 75, 90, 100, 1, 50, 49, 51, 99, 90)):
        head = V.jpeg_header(h, w, q)
        assert head == J.header(h, w, q, V.RESTART)
        theirs = pillow_jpeg(J.picture("ramp", h, w), q, V.RESTART)
        assert theirs.startswith(head)
    with pytest.raises(ValueError):
        V.jpeg_header(0, 5, 90)
    with pytest.raises(ValueError):
        V.jpeg_header(5, 65536, 90)


# ---- 3. planted faults: the comparison with Pillow notices each ------------------------------------------------------------------
PLANTED = {   # fault -> a case (h, w, content, quality, R) of test 1 whose file it changes
    "chroma_rows_before_downsample": (2, 16, "noise", 75, 16),     # an even height that is no multiple of 16
    "transformed_padding": (2, 16, "noise", 75, 16),               # the lower Y blocks of the MCU are dummy
    "bias_from_2": (2, 16, "noise", 90, 16),
    "quant_floor": (2, 16, "noise", 90, 16),
    "rst_no_wrap": (200, 40, "noise", 90, 3),                      # 39 MCUs: 13 intervals, the ninth marker is RST0 again
    "dc_no_reset": (17, 9, "noise", 75, 1),                        # two MCUs, an interval each
    "pad_zero": (1, 1, "noise", 75, 16),
    "missing_stuffing": (1, 1, "ramp", 100, 1),
    "missing_zrl": (8, 16, "noise", 5, 16),
    "eob_always": (2, 16, "noise", 90, 16),                        # quality 90 noise: blocks that end in a non-zero coefficient
}


def test_every_fault_is_planted():
    assert sorted(PLANTED) == sorted(J.FAULTS) and len(J.FAULTS) == 10
    assert all(case in set(cases()) for case in PLANTED.values())


@pytest.mark.parametrize("fault", J.FAULTS)
def test_planted_fault_is_noticed(pillow, fault):
    h, w, kind, q, R = PLANTED[fault]
    img = J.picture(kind, h, w)
    theirs = pillow_jpeg(img, q, R)
    assert J.encode(img, q, R) == theirs
    assert J.encode(img, q, R, faults=(fault,)) != theirs, f"{fault} does not change {PLANTED[fault]}"


# ---- 4. the container ------------------------------------------------------------------------------------------------------------
def ref_encoder(frames, quality):
    return (J.encode(np.asarray(f), quality) for f in frames)


@pytest.fixture(scope="module")
def avi(tmp_path_factory):
    """five frames of 33 x 50 whose files have odd and even lengths"""
    frames = [J.picture("noise", 33, 50, seed=s) for s in range(5)]
    files = [J.encode(f, 75) for f in frames]
    assert {len(f) & 1 for f in files} == {0, 1}, "the fixture needs odd and even chunk lengths"
    path = str(tmp_path_factory.mktemp("avi") / "clip.avi")
    assert V.write_mjpeg_avi(frames, path, fps=12, quality=75, encoder=ref_encoder) == path
    return path, files


def test_avi_round_trip(avi):
    from PIL import Image
    path, files = avi
    frames, info = V.read_mjpeg_avi(path, with_info=True)
    assert frames == files and V.read_mjpeg_avi(path) == files
    assert info == {"frames": 5, "fps": 12, "width": 50, "height": 33}
    for data in frames:
        im = Image.open(io.BytesIO(data))
        assert im.size == (50, 33)
        im.load()


def test_avi_layout(avi):
    """checked here by hand, independently of read_mjpeg_avi: padding, idx1, the header fields"""
    path, files = avi
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == len(data) - 8 and data[8:12] == b"AVI "
    movi = data.index(b"movi")
    assert data[movi - 8:movi - 4] == b"LIST"
    pos, where = movi + 4, []
    for f in files:
        assert data[pos:pos + 4] == b"00dc" and struct.unpack("<I", data[pos + 4:pos + 8])[0] == len(f)
        assert data[pos + 8:pos + 8 + len(f)] == f and pos % 2 == 0
        where.append((pos - movi, len(f)))
        pos += 8 + len(f)
        if len(f) & 1:
            assert data[pos] == 0
            pos += 1
    assert pos == movi + struct.unpack("<I", data[movi - 4:movi])[0] and data[pos:pos + 4] == b"idx1"
    assert struct.unpack("<I", data[pos + 4:pos + 8])[0] == 16 * len(files) and pos + 8 + 16 * len(files) == len(data)
    for i, (off, size) in enumerate(where):
        assert struct.unpack("<4sIII", data[pos + 8 + 16 * i:pos + 24 + 16 * i]) == (b"00dc", 0x10, off, size)
    avih = data.index(b"avih")
    fields = struct.unpack("<14I", data[avih + 8:avih + 64])
    assert fields[0] == 1000000 // 12 and fields[3] & 0x10 and fields[4] == 5 and fields[6] == 1 and fields[8:10] == (50, 33)
    strh = data.index(b"strh")
    assert data[strh + 8:strh + 16] == b"vidsMJPG" and struct.unpack("<III", data[strh + 28:strh + 40]) == (1, 12, 0)
    assert struct.unpack("<I", data[strh + 40:strh + 44])[0] == 5
    strf = data.index(b"strf")
    assert struct.unpack("<IiiHH4s", data[strf + 8:strf + 28]) == (40, 50, 33, 1, 24, b"MJPG")


def test_reader_fails_by_name(avi, tmp_path):
    path, files = avi
    data = open(path, "rb").read()

    def reading(blob):
        p = str(tmp_path / "broken.avi")
        with open(p, "wb") as fh:
            fh.write(blob)
        return V.read_mjpeg_avi(p)

    for cut in (1, 2, 16, len(files[-1]) + 90, len(data) - 20):
        with pytest.raises(V.AviError, match="RIFF size"):
            reading(data[:-cut])
    movi = data.index(b"movi")
    first = movi + 4
    for at, what in ((first + 4, "00dc"), (movi - 4, "movi|idx1|runs past"), (data.index(b"idx1") + 4, "idx1"),
                     (data.index(b"idx1") + 8 + 8, r"idx1\[0\]"), (data.index(b"idx1") + 8 + 16 + 12, r"idx1\[1\]"),
                     (data.index(b"avih") + 8 + 16, "dwTotalFrames"), (data.index(b"avih") + 4, "avih size"),
                     (data.index(b"strf") + 8 + 4, "strf")):
        blob = bytearray(data)
        blob[at] ^= 0x02
        with pytest.raises(V.AviError, match=what):
            reading(bytes(blob))
    assert isinstance(V.AviError("x"), ValueError)


def test_one_gibibyte_is_refused(tmp_path):
    big = b"\xff\xd8" + bytes(64 << 20) + b"\xff\xd9"
    calls = []

    def stub(frames, quality):
        for _ in frames:
            calls.append(1)
            yield big
    path = str(tmp_path / "big.avi")
    with pytest.raises(ValueError, match="1 GiB"):
        V.write_mjpeg_avi(range(40), path, fps=10, encoder=stub)
    assert len(calls) == 16 and not os.path.exists(path)
    with pytest.raises(ValueError, match="fps"):
        V.write_mjpeg_avi([], path, fps=2.5, encoder=stub)
    with pytest.raises(ValueError, match="no frames"):
        V.write_mjpeg_avi([], path, fps=2, encoder=stub)


def test_jpeg_folder(tmp_path):
    from PIL import Image
    frames = [J.picture("ramp", 17, 9, seed=s) for s in range(3)]
    folder = V.write_jpeg_frames(frames, str(tmp_path / "out" / "frames"), quality=90, encoder=ref_encoder)
    assert sorted(os.listdir(folder)) == ["00000.jpg", "00001.jpg", "00002.jpg"]
    assert Image.open(os.path.join(folder, "00002.jpg")).size == (9, 17)
