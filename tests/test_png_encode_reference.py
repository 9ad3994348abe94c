"""CPU: the restatement of the PNG encoder's bit-defined stages (tests/png_enc_ref.py) against png_ref's unfilter, zlib.crc32 and
Pillow; the host-built header against Pillow's; and planted single faults, which these same checks must notice."""
import io
import zlib

import numpy as np
import pytest

import png_enc_ref as E
import png_ref as R

SIZES = [(1, 1), (1, 5), (5, 1), (3, 67), (9, 14)]


def picture(h, w, bpp, seed):
    """smooth gradients with noise and a few flat runs: every filter wins some rows, predictors wrap around"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(3 * x + 5 * y * (c + 1) + rng.integers(0, 6, size=(h, w))) % 256 for c in range(bpp)], axis=-1)
    img[h // 2:, : w // 2] = 200
    if h > 2:
        img[1] = rng.integers(0, 256, size=(w, bpp))
    return img.astype(np.uint8)


def check_unfilter_round_trip():
    for h, w in SIZES:
        for bpp in (1, 3):
            img = picture(h, w, bpp, seed=10 * h + w + bpp)
            for kind in (0, 1, 2, 3, 4, E.ADAPTIVE):
                raw = E.filter_image(img, kind)
                assert len(raw) == h * (1 + w * bpp)
                if kind != E.ADAPTIVE:
                    assert set(raw[:: 1 + w * bpp]) == {kind}
                back, status = R.unfilter(raw, h, w, bpp)
                assert status == 0 and np.array_equal(back, img), (h, w, bpp, kind)
                assert E.filter_image_fast(img, kind) == raw, (h, w, bpp, kind)


def check_heuristic_on_hand_made_rows():
    zeros = [0] * 8
    # a constant row under a zero row: None costs 8 * 7, Sub 7, Up 56, Average 7 + 7 * 4 (7 - 3 = 4), Paeth 7 -> Sub (1) before Paeth (4)
    assert E.choose_filter([7] * 8, zeros, 1)[0] == 1
    # the same row again below it: Up costs 0, Sub 7, Average 4, Paeth 0 -> the tie goes to Up (2), not Paeth (4)
    assert E.choose_filter([7] * 8, [7] * 8, 1) == (2, [0] * 8)
    # all zeros: every filter costs 0 -> None
    assert E.choose_filter(zeros, zeros, 1)[0] == 0
    # 255 counts as |-1| = 1, 128 as 128: None on [255] * 8 costs 8, not 2040
    assert E.row_cost([255] * 8) == 8 and E.row_cost([128, 127, 129]) == 128 + 127 + 127
    # signed cost decides: None gives 250 -> |-6| = 6 a byte (48); Sub gives 250 then zeros (6) -> Sub
    assert E.choose_filter([250] * 8, zeros, 1)[0] == 1
    # a ramp under itself shifted: Average wins where left and up straddle the value
    cur, prev = [10, 20, 30, 40, 50, 60, 70, 80], [30, 40, 50, 60, 70, 80, 90, 100]
    costs = [E.row_cost(E.filter_row(k, cur, prev, 1)) for k in range(5)]
    assert E.choose_filter(cur, prev, 1)[0] == costs.index(min(costs))
    # three channels: the left neighbour is three bytes back
    assert E.filter_row(1, [1, 2, 3, 5, 7, 9], [0] * 6, 3) == [1, 2, 3, 4, 5, 6]


def check_paeth_tie_order():
    """the only ties whose order shows in the value: pb == pc < pa picks up (b) over up-left (c); pa == pc <= pb picks left (a)"""
    found_bc = found_ac = False
    for a in range(0, 12):
        for b in range(0, 12):
            for c in range(0, 12):
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                got = E.paeth(a, b, c)
                if pa <= pb and pa <= pc:
                    assert got == a
                    found_ac |= pa == pc and a != c
                elif pb <= pc:
                    assert got == b
                    found_bc |= pb == pc and b != c
                else:
                    assert got == c
    assert found_bc and found_ac


def check_crc_combination():
    data = bytes((37 * i + (i >> 3)) & 255 for i in range(41))
    want = zlib.crc32(data)
    assert E.crc_register(data, 0xFFFFFFFF) ^ 0xFFFFFFFF == want
    for cut in range(len(data) + 1):
        assert E.crc32_pieces(data, [cut]) == want, cut
    for cuts in ([], [0, 0], [5, 6, 7], [1, 20, 40, 41], list(range(1, 41))):
        assert E.crc32_pieces(data, cuts) == want, cuts
    assert E.crc32_pieces(b"", []) == 0 == zlib.crc32(b"")
    big = np.random.default_rng(3).integers(0, 256, size=5000, dtype=np.uint8).tobytes()
    assert E.crc32_pieces(big, list(range(64, 5000, 64))) == zlib.crc32(big)
    # the powers: x^8 is one byte of zeros through the register started at x^0
    assert E.x_pow8(0) == 0x80000000 and E.x_pow8(1) == E.crc_register(b"\x00", 0x80000000)
    assert E.gf_mul(E.x_pow8(5), E.x_pow8(9)) == E.x_pow8(14)


CHECKS = [check_unfilter_round_trip, check_heuristic_on_hand_made_rows, check_paeth_tie_order, check_crc_combination]


@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__)
def test_restatement(check):
    assert not E.FAULTS and not R.FAULTS
    check()


@pytest.mark.parametrize("fault,check", [
    ("paeth_tie", check_paeth_tie_order),
    ("average_up", check_unfilter_round_trip),
    ("cost_unsigned", check_heuristic_on_hand_made_rows),
    ("tie_highest", check_heuristic_on_hand_made_rows),
    ("pow_short", check_crc_combination),
    ("no_start_term", check_crc_combination),
])
def test_planted_faults_are_noticed(fault, check):
    E.FAULTS.add(fault)
    try:
        with pytest.raises(AssertionError):
            check()
    finally:
        E.FAULTS.discard(fault)
    check()


@pytest.mark.parametrize("mode,channels", [("L", 1), ("RGB", 3)])
def test_header_equals_pillows(mode, channels):
    from PIL import Image
    from dino_tracker_amd import png_out
    for h, w in ((1, 1), (5, 7), (480, 854), (65535, 1)):
        buf = io.BytesIO()
        Image.new(mode, (w, h)).save(buf, format="PNG")
        assert png_out.png_header(h, w, channels) == buf.getvalue()[:33], (mode, h, w)
    for bad in ((0, 4, 1), (4, 65536, 3), (4, 4, 2), (4, 4, 4)):
        with pytest.raises(ValueError):
            png_out.png_header(*bad)


def test_a_file_from_the_restated_stages_is_a_png():
    """filter_image + zlib + crc32_pieces, framed by hand: Pillow reads the image back, so the restatement describes the format"""
    import struct
    from PIL import Image
    from dino_tracker_amd import png_out
    for bpp in (1, 3):
        img = picture(9, 14, bpp, seed=4)
        z = zlib.compress(E.filter_image(img, E.ADAPTIVE), 1)
        body = b"IDAT" + z
        crc = E.crc32_pieces(body, [4, len(body) // 2])
        data = (png_out.png_header(9, 14, bpp) + struct.pack(">I", len(z)) + body + struct.pack(">I", crc) +
                struct.pack(">I", 0) + b"IEND" + struct.pack(">I", zlib.crc32(b"IEND")))
        chunks = E.walk(data)
        assert [k for k, *_ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and all(s == c for _, _, s, c in chunks)
        Image.open(io.BytesIO(data)).verify()
        got = np.asarray(Image.open(io.BytesIO(data)))
        assert np.array_equal(got.reshape(img.shape), img)


def test_cpu_tensors_are_refused():
    import torch
    from dino_tracker_amd import png_out
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        png_out.encode_png(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        png_out.deflate([b"abc"], device="cpu")
    with pytest.raises(ValueError):
        png_out.encode_png(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), filter="best")


def test_save_masks_switch_is_validated(monkeypatch, tmp_path):
    import torch
    from dino_tracker_amd import fg_mask, png_out
    monkeypatch.setattr(png_out, "write_png_frames", lambda *a, **k: pytest.fail("the default must not reach the device encoder"))
    mask = torch.zeros(2, 5, 6, dtype=torch.uint8)
    monkeypatch.delenv("DTK_PNG_ENCODE", raising=False)
    assert not fg_mask.png_encode_on_device()
    fg_mask.save_masks(mask, str(tmp_path / "m"))
    assert sorted(p.name for p in (tmp_path / "m").iterdir()) == ["00000.png", "00001.png"]
    monkeypatch.setenv("DTK_PNG_ENCODE", "gpu")
    with pytest.raises(ValueError):
        fg_mask.save_masks(mask, str(tmp_path / "n"))
