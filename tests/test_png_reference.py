"""CPU: the restatement of the PNG decoder (tests/png_ref.py) against zlib and Pillow, the chunk parser (dino_tracker_amd/png_in.py)
on files it must accept and decline, the palette table against Pillow's convert("L"), planted faults in the restatement, and the
shared stream-level core (csrc/inflate_core.h) as a stand-alone host program under the address and undefined-behaviour sanitisers.
Everything is an equality: the format is lossless."""
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_cases as C
import png_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pillow():
    return pytest.importorskip("PIL.Image")


def pillow_pixels(Image, data, mode=None):
    with Image.open(io.BytesIO(data)) as img:
        img.load()
        return np.asarray(img.convert(mode) if mode else img)


# ---- 1. inflate ------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_zlib_on_every_valid_case():
    seen = {"longest": {}, "distance": {}, "blocks": [0, 0, 0]}
    for name, stream, data in C.cases():
        assert zlib.decompress(stream) == data, name
        out, status, stats = R.inflate(stream, len(data))
        assert status == 0 and out == data, (name, status)
        raw, status, _ = R.inflate(stream[2:-4], len(data), wrapper=False)
        assert status == 0 and raw == data, (name, status)
        seen["longest"][name], seen["distance"][name] = stats["longest_code"], stats["largest_distance"]
        seen["blocks"] = [a + b for a, b in zip(seen["blocks"], stats["blocks"])]
    # the cases reach what they are there for
    assert seen["longest"]["huffman_only_fibonacci"] == 15
    assert seen["distance"]["hand_distance_32768"] == 32768 and seen["distance"]["z_rle_constant"] == 1
    assert all(n > 0 for n in seen["blocks"]), seen["blocks"]
    assert R.inflate(C.cases()[2][1], 70001)[2]["blocks"][0] == 2          # level 0: two stored blocks


def test_restatement_reports_the_expected_status_on_every_damaged_case():
    for name, stream, expected, want, zlib_raises in C.damaged():
        out, status, _ = R.inflate(stream, expected)
        assert status == want and len(out) == expected, (name, status, want)
        if zlib_raises:
            with pytest.raises(zlib.error):
                zlib.decompress(stream)
        else:
            assert len(zlib.decompress(stream)) != expected
    # what was decoded before the fault stays, the rest is zero
    name, stream, expected, want, _ = C.damaged()[-1]
    out, _, _ = R.inflate(stream, expected)
    assert want == R.S_DISTANCE and out[:32767] == C.random_bytes(32767, 3) and out[32767:] == bytes(258)


def test_adler32_restatement():
    for data in (b"", b"a", C.random_bytes(70001, 2)):
        assert R.adler32(data) == zlib.adler32(data)


# ---- 2. files --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4, "mixed"])
def test_written_files_decode_equal_under_pillow_and_the_restatement(pillow, filt):
    rng = np.random.default_rng(7)
    palette = rng.integers(0, 256, size=3 * 200, dtype=np.uint8).tobytes()
    for name, img, pal in (("L", C.picture(37, 29, 1), None), ("RGB", C.picture(37, 29, 3), None),
                           ("P", rng.integers(0, 200, size=(37, 29), dtype=np.uint8), palette)):
        filters = C.filter_sequence(37, seed=3) if filt == "mixed" else filt
        whole = C.write_png(img, filters, palette=pal)
        n = sum(len(body) for kind, body in R.chunks(whole) if kind == b"IDAT")
        for split in ((), (n // 2,), (0, 1, 2, 2, n // 3, n - 1)):      # 1, 2 and 7 pieces: empty ones, a cut inside a code
            data = C.write_png(img, filters, idat_split=split, palette=pal)
            assert sum(kind == b"IDAT" for kind, _ in R.chunks(data)) == len(split) + 1
            px, status, _, plte = R.decode_png(data)
            assert status == 0 and np.array_equal(px.reshape(img.shape), img), (name, filt, split)
            assert np.array_equal(pillow_pixels(pillow, data), img), (name, filt, split)
            assert (plte == pal) if pal else plte is None


@pytest.mark.parametrize("level", [1, 6, 9])
def test_pillow_written_files(pillow, level):
    for img in (C.picture(41, 53, 3, seed=1), C.picture(41, 53, 1, seed=2)):
        buf = io.BytesIO()
        pillow.fromarray(img).save(buf, format="PNG", compress_level=level)
        px, status, _, _ = R.decode_png(buf.getvalue())
        assert status == 0 and np.array_equal(px.reshape(img.shape), img)


def test_a_filter_byte_above_4_is_flagged():
    raw = bytes([0, 1, 2, 3, 7, 4, 5, 6])
    px, status = R.unfilter(raw, 2, 3, 1)
    assert status == R.PNG_S_FILTER and px[1, :, 0].tolist() == [4, 5, 6]


# ---- 3. the parser ---------------------------------------------------------------------------------------------------------------
def _save(Image, array, mode=None, **kw):
    buf = io.BytesIO()
    img = Image.fromarray(array, mode) if mode else Image.fromarray(array)
    img.save(buf, format="PNG", **kw)
    return buf.getvalue()


def test_parser_accepts_and_declines_with_the_reason(pillow):
    from dino_tracker_amd import png_in
    rgb, grey = C.picture(19, 23, 3), C.picture(19, 23, 1)
    pal = bytes(range(256)) * 3
    for data, mode in ((C.write_png(rgb, 4), "RGB"), (C.write_png(grey, 3), "L"), (C.write_png(grey, 1, palette=pal[:300]), "P"),
                       (_save(pillow, rgb), "RGB"), (_save(pillow, grey), "L")):
        h, why = png_in.parse_png(data)
        assert h is not None and (h.height, h.width, h.mode) == (19, 23, mode), why
        assert (h.palette == pal[:300]) if mode == "P" else h.palette is None
        joined = b"".join(data[o:o + n] for o, n in h.idat.tolist())
        px, status = R.unfilter(zlib.decompress(joined), 19, 23, h.bpp)
        assert status == 0 and np.array_equal(px.reshape((rgb if mode == "RGB" else grey).shape), rgb if mode == "RGB" else grey)
    # IDAT ranges: any number of chunks, empty ones included
    data = C.write_png(rgb, 2, idat_split=(0, 5, 5, 40))
    h, _ = png_in.parse_png(data)
    assert h.idat[:, 1].tolist()[:4] == [0, 5, 0, 35] and h.idat.shape[0] == 5
    assert zlib.decompress(b"".join(data[o:o + n] for o, n in h.idat.tolist())) == C.filter_rows(rgb, 2)

    wide = (np.arange(19 * 23, dtype=np.uint16).reshape(19, 23) * 97)
    rgba = np.dstack([rgb, grey])
    la = np.dstack([grey, grey])
    p_img = pillow.fromarray(grey).convert("P")
    buf = io.BytesIO()
    p_img.save(buf, format="PNG", transparency=3)
    good = C.write_png(rgb, 1)
    bad_crc = bytearray(good)
    bad_crc[20] ^= 1                                                   # inside IHDR's payload
    bad_plte = bytearray(C.write_png(grey, 1, palette=pal[:300]))
    bad_plte[33 + 8 + 5] ^= 1
    gap = C.SIGNATURE + good[8:33]
    body = [c for c in R.chunks(C.write_png(rgb, 1, idat_split=(10,)))]
    gap += C.chunk(*body[1]) + C.chunk(b"tEXt", b"k\x00v") + C.chunk(*body[2]) + C.chunk(b"IEND", b"")
    sub = C.SIGNATURE + C.chunk(b"IHDR", struct.pack(">IIBBBBB", 8, 8, 4, 0, 0, 0, 0)) + good[33:]
    for data, word in ((_save(pillow, wide), "bit depth 16"), (_save(pillow, rgba), "RGBA"), (_save(pillow, la), "alpha"),
                       (_interlaced(good), "interlaced"),
                       (buf.getvalue(), "tRNS"), (C.write_png(rgb, 1, extra=[(b"tRNS", bytes(6))]), "tRNS"),
                       (bytes(bad_crc), "IHDR: CRC"), (bytes(bad_plte), "PLTE: CRC"), (good[:-12], "no IEND"),
                       (good[:-20], "runs past the file"), (b"\xff\xd8" + good, "signature"), (gap, "not consecutive"),
                       (sub, "bit depth 4")):
        h, why = png_in.parse_png(data)
        assert h is None and word in why, (word, why)
    plan, why = png_in.plan_png([good, C.write_png(C.picture(19, 24, 3), 1)])
    assert plan is None and "file 1: 19 x 24 RGB, file 0 is 19 x 23 RGB" in why
    plan, why = png_in.plan_png([good, C.write_png(grey, 1)])
    assert plan is None and "file 1: 19 x 23 L" in why
    plan, why = png_in.plan_png([good, C.write_png(rgb, 3, idat_split=(7,))])
    assert why is None and plan.frames == 2 and plan.streams[:, 3].tolist() == [19 * 70] * 2 and plan.streams[1, 2] == 19 * 70
    pinned, plan2, datas, why = png_in.read_pinned([good, C.write_png(rgb, 3, idat_split=(7,))])
    assert why is None and len(datas) == 2
    for f, want in enumerate((C.filter_rows(rgb, 1), C.filter_rows(rgb, 3))):
        o, n = plan2.streams[f, :2].tolist()
        assert zlib.decompress(pinned.numpy()[o:o + n].tobytes()) == want


def _interlaced(good):
    """the IHDR of `good` with the interlace method set to 1 (and its CRC recomputed): the parser declines before it reads on"""
    ihdr = bytearray(good[16:29])
    ihdr[12] = 1
    return C.SIGNATURE + C.chunk(b"IHDR", bytes(ihdr)) + good[33:]


def test_palette_table_equals_pillow_convert_l(pillow):
    from dino_tracker_amd import png_in
    rng = np.random.default_rng(11)
    for n in (256, 256, 200, 1):
        pal = rng.integers(0, 256, size=3 * n, dtype=np.uint8).tobytes()
        idx = rng.integers(0, n, size=(16, 16), dtype=np.uint8)
        idx.flat[:n] = np.arange(n, dtype=np.uint8)[:256]
        data = C.write_png(idx, 0, palette=pal)
        want = pillow_pixels(pillow, data, "L")
        lut = png_in.palette_to_l(pal)
        assert np.array_equal(lut[idx], want) and np.array_equal(R.palette_to_l(pal), lut)
    # the two entries the rounding was first confirmed on, and the extremes
    pal = bytes([255, 255, 255, 0, 0, 0, 255, 0, 0, 1, 2, 3])
    assert png_in.palette_to_l(pal)[:4].tolist() == [255, 0, 76, 2]


# ---- 4. planted faults: each is noticed ------------------------------------------------------------------------------------------
@pytest.fixture
def planted():
    yield R.FAULTS
    R.FAULTS.clear()


def _all_agree():
    for name, stream, data in C.cases():
        out, status, _ = R.inflate(stream, len(data))
        if status != 0 or out != data:
            return False
    img = C.picture(30, 17, 3, seed=4)
    for filt in (3, 4):
        px, status, _, _ = R.decode_png(C.write_png(img, filt))
        if status != 0 or not np.array_equal(px, img):
            return False
    return True


def test_without_faults_everything_agrees():
    assert _all_agree()


@pytest.mark.parametrize("fault", ["paeth_tie", "average_up", "length_base", "dist_extra_msb", "repeat16_zero"])
def test_planted_faults_are_noticed(planted, fault):
    planted.add(fault)
    assert not _all_agree(), fault


# ---- 5. the shared core under the sanitisers -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler (CXX, g++, clang++) to build tests/host/inflate_host.cpp")
    exe = str(tmp_path_factory.mktemp("host") / "inflate_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-o", exe, os.path.join(HERE, "host", "inflate_host.cpp")], check=True)
    return exe


def case_file(stream, expected, wrapper=1):
    return b"INFC" + struct.pack("<iq", wrapper, expected) + stream


def test_shared_core_decodes_every_case_under_the_sanitisers(host_program, tmp_path):
    jobs = [(name, stream, len(data), 1, 0, zlib.crc32(data)) for name, stream, data in C.cases()]
    jobs += [(name + "_raw", stream[2:-4], len(data), 0, 0, zlib.crc32(data)) for name, stream, data in C.cases()]
    for name, stream, expected, want, _ in C.damaged():
        out, status, _ = R.inflate(stream, expected)
        if want != R.S_ADLER:                       # the trailer is dtk_adler32's business, not the core's
            jobs.append((name, stream, expected, 1, want, zlib.crc32(out)))
    paths = []
    for name, stream, expected, wrapper, _, _ in jobs:
        path = tmp_path / f"{name}.case"
        path.write_bytes(case_file(stream, expected, wrapper))
        paths.append(str(path))
    done = subprocess.run([host_program] + paths, capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    lines = done.stdout.splitlines()
    assert len(lines) == len(jobs)
    for (name, _, _, _, want, crc), line in zip(jobs, lines):
        status, got_crc, longest = line.split()
        assert int(status) == want and int(got_crc, 16) == crc, (name, line, want, f"{crc:08x}")
        if name == "huffman_only_fibonacci":
            assert int(longest) == 15
