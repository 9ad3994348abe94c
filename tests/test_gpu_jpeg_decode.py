"""GPU: the device JPEG decoder (csrc/jpeg_decode.hip, csrc/jpeg_entropy.h, dino_tracker_amd/video_in.py) against the numpy
restatement of docs/JPEG_DECODE.md (tests/jpeg_dec_ref.py) and against Pillow's decoder -- never against the code under test.
Everything is an equality: the arithmetic is integer.  The restatement's own agreement with Pillow over many more files is the CPU
file's business (tests/test_jpeg_decode_reference.py).

Sizes (H x W): one pixel; 17 x 17 and 15 x 33 (odd chroma height, partial last MCU both ways); 2 x 16 (one chroma row: both vertical
neighbours clamp); 31 x 47; 32 x 854 (54 MCUs per row, two chroma block rows, more than one restart interval of 16)."""
import os

import numpy as np
import pytest
import torch

import jpeg_dec_cases as C
import jpeg_dec_ref as D
import jpeg_ref as J

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (17, 17), (15, 33), (2, 16), (31, 47), (32, 854)]
POISON = 0xA5
GUARD = 4096   # bytes
HORSEJUMP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "horsejump_00000.jpg")

_REF = {}


def ref(data):
    """(coefficients, pixels) of the restatement for one file, computed once and never modified"""
    if data not in _REF:
        coef, px = D.coefficients(data), D.decode(data)
        coef.setflags(write=False)
        px.setflags(write=False)
        _REF[data] = (coef, px)
    return _REF[data]


def guarded(nbytes):
    """(whole buffer filled with POISON, the 256-byte aligned view of `nbytes` between two guard bands, its start)"""
    whole = torch.full((GUARD + nbytes + 256 + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(whole.data_ptr() + GUARD)) % 256
    return whole, whole[start:start + nbytes], start


def bands_intact(whole, start, nbytes):
    return bool((whole[:start] == POISON).all()) and bool((whole[start + nbytes:] == POISON).all())


def raw_decode(files):
    """both entry points through ctypes on guarded buffers -> (coef int16 [F, MCUs, 6, 64], status [F], pixels uint8 [F, H, W, 3],
    every guard band intact)"""
    from dino_tracker_amd import ops, video_in
    from dino_tracker_amd._lib import lib
    plan, why = video_in.plan_jpeg(files)
    assert plan is not None, why
    F, H, W = plan.frames, plan.height, plan.width
    mcus = -(-H // 16) * -(-W // 16)
    stream = torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy()).to(DEV)
    seg = torch.from_numpy(plan.segments).to(DEV)
    huff, qt = torch.from_numpy(plan.huffman).to(DEV), torch.from_numpy(plan.qtables).to(DEV)
    sizes = (F * mcus * 768, 4 * F, F * H * W * 3, ops.jpeg_decode_workspace_bytes(F, H, W))
    assert sizes[3] > 0 and sizes[3] % 256 == 0
    bufs = [guarded(n) for n in sizes]
    coef, status, out, ws = (b[1] for b in bufs)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib().dtk_jpeg_decode_coefficients(stream.data_ptr(), stream.numel(), seg.data_ptr(), plan.segments.ctypes.data,
                                            plan.segments.shape[0], huff.data_ptr(), F, H, W, coef.data_ptr(), status.data_ptr(), st)
    assert rc == 0, lib().dtk_last_error()
    rc = lib().dtk_jpeg_pixels(coef.data_ptr(), qt.data_ptr(), F, H, W, out.data_ptr(), status.data_ptr(), ws.data_ptr(), st)
    assert rc == 0, lib().dtk_last_error()
    torch.cuda.synchronize()
    intact = all(bands_intact(b[0], b[2], n) for b, n in zip(bufs, sizes))
    return (coef.cpu().numpy().view(np.int16).reshape(F, mcus, 6, 64), status.cpu().numpy().view(np.int32),
            out.cpu().numpy().reshape(F, H, W, 3), intact)


# ---- 1. coefficients and pixels, one frame and three ------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_frames_equal_the_restatement_and_pillow(size):
    h, w = size
    for kind, q in (("noise", 90), ("ramp", 100), ("checker", 5), ("pm1", 75)):
        for name, data in C.variants(J.picture(kind, h, w), q):
            want_coef, want_px = ref(data)
            coef, status, px, intact = raw_decode([data])
            assert intact and status.tolist() == [0], (size, kind, q, name, status)
            assert np.array_equal(coef[0], want_coef), (size, kind, q, name)
            assert np.array_equal(px[0], want_px) and np.array_equal(px[0], C.pillow_decode(data)), (size, kind, q, name)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_frames_with_their_own_tables(size):
    """optimised Huffman tables on noise and on a ramp, the default ones on a checker; three qualities: three sets of tables"""
    from dino_tracker_amd import video_in
    h, w = size
    files = [C.pillow_encode(J.picture("noise", h, w, seed=1), 90, optimize=True),
             C.pillow_encode(J.picture("ramp", h, w), 100, optimize=True), C.pillow_encode(J.picture("checker", h, w), 50)]
    coef, status, px, intact = raw_decode(files)
    assert intact and status.tolist() == [0, 0, 0]
    for f, data in enumerate(files):
        want_coef, want_px = ref(data)
        assert np.array_equal(coef[f], want_coef) and np.array_equal(px[f], want_px), (size, f)
        assert np.array_equal(px[f], C.pillow_decode(data)), (size, f)
    # the public entry points: the same frames, from bytes
    frames, st = video_in.decode_jpeg(files, DEV, with_status=True)
    assert frames.dtype == torch.uint8 and frames.is_cuda and st.tolist() == [0, 0, 0]
    assert torch.equal(frames.cpu(), torch.from_numpy(px.copy()))
    c2, s2, plan = video_in.decode_jpeg_coefficients(files, DEV)
    assert torch.equal(c2.cpu(), torch.from_numpy(coef.copy())) and s2.tolist() == [0, 0, 0] and plan.frames == 3


def test_a_real_frame_without_restart_markers():
    """854 x 480 in ONE segment of 3 240 MCUs and 65 kB: the staging buffer is refilled many times"""
    from dino_tracker_amd import video_in
    with open(HORSEJUMP, "rb") as fh:
        data = fh.read()
    want = torch.from_numpy(C.pillow_decode(data))
    frames, status = video_in.decode_jpeg([HORSEJUMP, data], DEV, fallback=False, with_status=True)   # a path and a byte string
    assert status.tolist() == [0, 0]
    assert torch.equal(frames[0].cpu(), want) and torch.equal(frames[1].cpu(), want)
    coef, _, _ = video_in.decode_jpeg_coefficients([data], DEV)
    assert np.array_equal(coef[0].cpu().numpy(), ref(data)[0])


def test_device_round_trip():
    """ops.jpeg_encode -> the decoder's coefficients = ops.jpeg_coefficients of the same frames"""
    from dino_tracker_amd import ops, video_in, video_out
    imgs = np.stack([J.picture(kind, 33, 70, seed=s) for kind, s in (("noise", 0), ("ramp", 0), ("noise", 2))])
    frames = torch.from_numpy(imgs).to(DEV)
    for q in (50, 90):
        qt = torch.from_numpy(video_out.quant_tables(q)).to(DEV)
        files = list(video_out.jpeg_files(frames, q))
        coef, status, _ = video_in.decode_jpeg_coefficients(files, DEV)
        assert status.tolist() == [0, 0, 0] and torch.equal(coef, ops.jpeg_coefficients(frames, qt))


# ---- 2. damaged streams (the cases the stand-alone host program passes on the CPU) -------------------------------------------------
@pytest.mark.parametrize("case", range(3), ids=lambda i: ("truncated", "flipped_bit", "unknown_code")[i])
def test_damaged_frame_is_reported_and_its_neighbours_are_not(case, tmp_path, monkeypatch):
    from dino_tracker_amd import video_in, video_io
    from dino_tracker_amd.train import load_video as host_load_video
    name, bad = C.damaged()[case]
    good = [C.good_file(seed=1), C.good_file(seed=2)]
    files = [good[0], bad, good[1]]
    coef, status, px, intact = raw_decode(files)
    assert intact and status[0] == 0 and status[2] == 0 and status[1] != 0, status
    if name in C.STATUS:
        assert status[1] == C.STATUS[name]
    for f, data in ((0, good[0]), (2, good[1])):
        assert np.array_equal(coef[f], ref(data)[0]) and np.array_equal(px[f], C.pillow_decode(data))
    # load_video: what the host path returns, or what it raises
    folder = tmp_path / "video"
    folder.mkdir()
    for t, data in enumerate(files):
        (folder / f"{t:05d}.jpg").write_bytes(data)
    try:
        want = host_load_video(str(folder), resize=(20, 30))
    except Exception as e:   # noqa: BLE001
        with pytest.raises(type(e)):
            video_io.load_video(str(folder), resize=(20, 30), device=DEV)
        return
    assert torch.equal(video_io.load_video(str(folder), resize=(20, 30), device=DEV).cpu(), want)
    frames, st = video_in.decode_jpeg(files, DEV, with_status=True)
    assert st[1] != 0 and np.array_equal(frames[1].cpu().numpy(), C.pillow_decode(bad))


def test_refusals_write_nothing():
    from dino_tracker_amd import ops, video_in
    from dino_tracker_amd._lib import lib
    h = lib()
    whole, buf, start = guarded(1 << 16)
    p = buf.data_ptr()
    seg = np.array([[0, 0, 64, 0, 1]], dtype=np.int64)
    sp = seg.ctypes.data
    for F, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 65536, 8), (1, 8, 65536), (-1, 8, 8)):
        assert h.dtk_jpeg_decode_workspace_bytes(F, H, W) == 0
        assert h.dtk_jpeg_decode_coefficients(p, 64, p, sp, 1, p, F, H, W, p, p, None) == -1 and b"jpeg_decode_coefficients" in h.dtk_last_error()
        assert h.dtk_jpeg_pixels(p, p, F, H, W, p, p, p, None) == -1 and b"jpeg_pixels" in h.dtk_last_error()
    for hole in (0, 2, 3, 5, 9, 10):
        args = [p, 64, p, sp, 1, p, 1, 8, 8, p, p, None]
        args[hole] = None
        assert h.dtk_jpeg_decode_coefficients(*args) == -1 and b"null pointer" in h.dtk_last_error()
    for hole in (0, 1, 5, 7):
        args = [p, p, 1, 8, 8, p, p, p, None]
        args[hole] = None
        assert h.dtk_jpeg_pixels(*args) == -1 and b"null pointer" in h.dtk_last_error()
    assert h.dtk_jpeg_decode_coefficients(p, 0, p, sp, 1, p, 1, 8, 8, p, p, None) == -1
    assert h.dtk_jpeg_decode_coefficients(p, 64, p, sp, 0, p, 1, 8, 8, p, p, None) == -1
    for row in ([1, 0, 64, 0, 1], [-1, 0, 64, 0, 1], [0, 1, 64, 0, 1], [0, -1, 8, 0, 1], [0, 0, 65, 0, 1], [0, 0, -1, 0, 1],
                [0, 0, 64, 1, 1], [0, 0, 64, 0, 2], [0, 0, 64, 0, 0], [0, 0, 64, -1, 1]):
        bad = np.array([row], dtype=np.int64)
        assert h.dtk_jpeg_decode_coefficients(p, 64, p, bad.ctypes.data, 1, p, 1, 8, 8, p, p, None) == -1
        assert b"does not fit" in h.dtk_last_error()
    torch.cuda.synchronize()
    assert bool((whole == POISON).all())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video_in.decode_jpeg([C.good_file()], "cpu")
    with pytest.raises(ValueError, match="progressive"):
        video_in.decode_jpeg([C.pillow_encode(J.picture("noise", 16, 16), 90, progressive=True)], DEV)
    with pytest.raises(RuntimeError, match="segments"):
        ops.jpeg_decode_coefficients(torch.zeros(8, dtype=torch.uint8, device=DEV), np.zeros((1, 4), np.int64),
                                     torch.zeros((1, 3, 2, 272), dtype=torch.uint8, device=DEV), 8, 8)


def test_device_copy_of_the_segment_table_is_checked_too():
    """the kernel repeats the range check on ITS copy of the table: an entry that does not fit decodes nothing"""
    from dino_tracker_amd._lib import lib
    data = C.good_file()
    from dino_tracker_amd import video_in
    plan, _ = video_in.plan_jpeg([data])
    stream = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(DEV)
    huff = torch.from_numpy(plan.huffman).to(DEV)
    lying = plan.segments.copy()
    lying[0, 2] = len(data) + 1000          # the device copy claims bytes beyond the stream
    whole, coef, start = guarded(6 * 768)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = lib().dtk_jpeg_decode_coefficients(stream.data_ptr(), len(data), torch.from_numpy(lying).to(DEV).data_ptr(),
                                            plan.segments.ctypes.data, 1, huff.data_ptr(), 1, 31, 47, coef.data_ptr(), status.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == [C.S_SEGMENT] and bool((whole == POISON).all())


# ---- 3. the wiring -----------------------------------------------------------------------------------------------------------------
def _folder(path, files, suffix=".jpg"):
    path.mkdir()
    for t, data in enumerate(files):
        (path / f"{t:05d}{suffix}").write_bytes(data)
    return str(path)


def test_load_video_takes_the_device_decoder(tmp_path, monkeypatch):
    from PIL import Image
    from dino_tracker_amd import video_in, video_io
    from dino_tracker_amd.train import load_video as host_load_video
    imgs = [J.picture("noise", 48, 64, seed=s) for s in range(3)]
    folder = _folder(tmp_path / "jpg", [C.pillow_encode(img, 90) for img in imgs])
    want = host_load_video(folder, resize=(28, 42))
    calls = []
    original = video_in.decode_planned
    monkeypatch.setattr(video_in, "decode_planned", lambda *a, **k: calls.append(1) or original(*a, **k))
    for mode, used in ((None, 1), ("device", 1), ("host", 0)):
        calls.clear()
        if mode is None:
            monkeypatch.delenv("DTK_JPEG_DECODE", raising=False)
        else:
            monkeypatch.setenv("DTK_JPEG_DECODE", mode)
        got = video_io.load_video(folder, resize=(28, 42), device=DEV)
        assert len(calls) == used and got.is_cuda and torch.equal(got.cpu(), want), mode
        assert torch.equal(video_io.load_video(folder, device=DEV, num_frames=2).cpu(), host_load_video(folder)[:2])
    monkeypatch.setenv("DTK_JPEG_DECODE", "sometimes")
    with pytest.raises(ValueError, match="DTK_JPEG_DECODE"):
        video_io.load_video(folder, device=DEV)
    monkeypatch.delenv("DTK_JPEG_DECODE")
    # a mixed folder, and a folder of JPEGs the device does not decode: today's path
    calls.clear()
    mixed = tmp_path / "mixed"
    _folder(mixed, [C.pillow_encode(img, 90) for img in imgs[:2]])
    Image.fromarray(imgs[2]).save(str(mixed / "00002.png"))
    assert torch.equal(video_io.load_video(str(mixed), resize=(28, 42), device=DEV).cpu(), host_load_video(str(mixed), resize=(28, 42)))
    prog = _folder(tmp_path / "prog", [C.pillow_encode(img, 90, progressive=True) for img in imgs])
    assert torch.equal(video_io.load_video(prog, resize=(28, 42), device=DEV).cpu(), host_load_video(prog, resize=(28, 42)))
    assert not calls


def test_avi_and_frame_folder_re_enter_on_the_device(tmp_path):
    from dino_tracker_amd import video_io, video_out
    from dino_tracker_amd.train import load_video as host_load_video
    imgs = np.stack([J.picture(kind, 33, 70, seed=s) for kind, s in (("noise", 0), ("ramp", 0), ("checker", 0))])
    path = video_out.write_mjpeg_avi(torch.from_numpy(imgs).to(DEV), str(tmp_path / "v.avi"), fps=5, quality=75)
    files = video_out.read_mjpeg_avi(path)
    frames, info = video_out.read_mjpeg_avi(path, with_info=True, device=DEV)
    assert info["frames"] == 3 and frames.is_cuda and tuple(frames.shape) == (3, 33, 70, 3)
    for f, data in enumerate(files):
        assert np.array_equal(frames[f].cpu().numpy(), C.pillow_decode(data))
    folder = video_out.write_jpeg_frames(torch.from_numpy(imgs).to(DEV), str(tmp_path / "frames"), quality=75)
    assert torch.equal(video_io.load_video(folder, device=DEV).cpu(), host_load_video(folder))
