"""GPU: the device JPEG decoder on gray, 4:4:4 and 4:2:2 files, and on 4:2:0 files too narrow for the "fancy" upsampling
(csrc/jpeg_decode.hip, csrc/jpeg_entropy.h, dino_tracker_amd/video_in.py), against the numpy restatement of docs/JPEG_DECODE.md
(tests/jpeg_sampling_ref.py) and against Pillow's decoder -- never against the code under test.  Everything is an equality: the
arithmetic is integer.  The restatement's own agreement with Pillow over many more files is the CPU file's business
(tests/test_jpeg_sampling_reference.py).

Sizes (H x W): one pixel; 5 x 4 and 4 x 5 (chroma planes 2 and 3 samples wide: replication against the filter); 9 x 17, 17 x 33 and
31 x 47 (partial last MCUs both ways, several MCU rows); 40 x 200 (25 MCUs per row at 4:4:4, more than one restart interval)."""
import numpy as np
import pytest
import torch

import jpeg_sampling_cases as SC
import jpeg_sampling_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (5, 4), (4, 5), (9, 17), (17, 33), (31, 47), (40, 200)]
NEW = (R.GRAY, R.S444, R.S422)
POISON = 0xA5
GUARD = 4096   # bytes
name_of = R.NAMES.get

_REF = {}


def ref(data):
    """(coefficients, pixels) of the restatement for one file, computed once and never modified"""
    if data not in _REF:
        coef, px = R.coefficients(data), R.decode(data)
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
    """the sampled entry points through ctypes on guarded buffers -> (coef int16 [F, MCUs, B, 64], status [F], pixels uint8
    [F, H, W, 3] or [F, H, W], every guard band around coefficients, status, output and planes intact)"""
    from dino_tracker_amd import ops, video_in
    from dino_tracker_amd._lib import lib
    plan, why = video_in.plan_jpeg_sampled(files)
    assert plan is not None, why
    F, H, W, S = plan.frames, plan.height, plan.width, plan.sampling
    B = R.blocks_per_mcu(S)
    mh, mw = R.mcu_grid(H, W, S)
    mcus, C_out = mh * mw, (1 if S == R.GRAY else 3)
    stream = torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy()).to(DEV)
    seg = torch.from_numpy(plan.segments).to(DEV)
    huff, qt = torch.from_numpy(plan.huffman).to(DEV), torch.from_numpy(plan.qtables).to(DEV)
    sizes = (F * mcus * B * 128, 4 * F, F * H * W * C_out, ops.jpeg_decode_workspace_bytes(F, H, W, S))
    assert sizes[3] >= F * mcus * B * 64 and sizes[3] % 256 == 0
    bufs = [guarded(n) for n in sizes]
    coef, status, out, ws = (b[1] for b in bufs)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib().dtk_jpeg_decode_coefficients_sampled(S, stream.data_ptr(), stream.numel(), seg.data_ptr(), plan.segments.ctypes.data,
                                                    plan.segments.shape[0], huff.data_ptr(), F, H, W, coef.data_ptr(),
                                                    status.data_ptr(), st)
    assert rc == 0, lib().dtk_last_error()
    rc = lib().dtk_jpeg_pixels_sampled(S, coef.data_ptr(), qt.data_ptr(), F, H, W, out.data_ptr(), status.data_ptr(), ws.data_ptr(), st)
    assert rc == 0, lib().dtk_last_error()
    torch.cuda.synchronize()
    intact = all(bands_intact(b[0], b[2], n) for b, n in zip(bufs, sizes))
    px = out.cpu().numpy().reshape((F, H, W) if S == R.GRAY else (F, H, W, 3))
    return coef.cpu().numpy().view(np.int16).reshape(F, mcus, B, 64), status.cpu().numpy().view(np.int32), px, intact


# ---- 1. coefficients and pixels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sampling", NEW, ids=name_of)
def test_frames_equal_the_restatement_and_pillow(sampling, size):
    from dino_tracker_amd import video_in
    h, w = size
    for name, data in SC.variants(SC.picture("noise", h, w, sampling), sampling, 75):
        frames = video_in.decode_jpeg([data], DEV)          # the public entry point first: it names what it does not decode
        assert tuple(frames.shape) == ((1, h, w, 1) if sampling == R.GRAY else (1, h, w, 3))
        want_coef, want_px = ref(data)
        assert np.array_equal(frames[0].cpu().numpy().reshape(want_px.shape), want_px), (size, name)
        coef, status, px, intact = raw_decode([data])
        assert intact and status.tolist() == [0], (size, name, status)
        assert np.array_equal(coef[0], want_coef), (size, name)
        assert np.array_equal(px[0], SC.pillow_decode(data)) and np.array_equal(px[0], want_px), (size, name)


@pytest.mark.parametrize("size", [(3, 1), (5, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_narrow_420_frames_are_replicated(size):
    """a 4:2:0 chroma plane at most two samples wide is not filtered, through the entry points that were there before as well"""
    from dino_tracker_amd import video_in
    from dino_tracker_amd._lib import lib
    h, w = size
    for name, data in SC.variants(SC.picture("noise", h, w, R.S420), R.S420, 75):
        want = SC.pillow_decode(data)
        coef, status, px, intact = raw_decode([data])
        assert intact and status.tolist() == [0] and np.array_equal(coef[0], ref(data)[0])
        assert np.array_equal(px[0], want) and np.array_equal(ref(data)[1], want), (size, name)
        plan, why = video_in.plan_jpeg([data])
        assert plan is not None, why
        c = torch.from_numpy(coef.copy()).to(DEV)
        qt = torch.from_numpy(plan.qtables).to(DEV)
        out = torch.empty((1, h, w, 3), dtype=torch.uint8, device=DEV)
        ws = torch.empty(lib().dtk_jpeg_decode_workspace_bytes(1, h, w), dtype=torch.uint8, device=DEV)
        rc = lib().dtk_jpeg_pixels(c.data_ptr(), qt.data_ptr(), 1, h, w, out.data_ptr(), None, ws.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and np.array_equal(out[0].cpu().numpy(), want), (size, name)


@pytest.mark.parametrize("sampling", NEW, ids=name_of)
def test_one_segment_larger_than_the_staging_buffer(sampling):
    """40 x 200 noise at quality 100 without restart markers: the scan is several times the 4 KiB staging buffer, refilled with B != 6"""
    from dino_tracker_amd import video_in
    data = SC.encode(SC.picture("noise", 40, 200, sampling), sampling, 100)
    h, why = video_in.parse_jpeg_sampled(data)
    assert h is not None and h.segments.shape[0] == 1 and int(h.segments[0, 1]) > 2 * 4096, why
    coef, status, px, intact = raw_decode([data])
    assert intact and status.tolist() == [0]
    assert np.array_equal(coef[0], ref(data)[0]) and np.array_equal(px[0], SC.pillow_decode(data))


@pytest.mark.parametrize("sampling", NEW, ids=name_of)
def test_three_frames_with_their_own_tables(sampling):
    """the default Huffman tables, optimised ones, another quality: three sets of tables in one call"""
    from dino_tracker_amd import video_in
    h, w = 17, 33
    files = [SC.encode(SC.picture("noise", h, w, sampling, seed=1), sampling, 90),
             SC.encode(SC.picture("ramp", h, w, sampling), sampling, 100, optimize=True),
             SC.encode(SC.picture("noise", h, w, sampling, seed=2), sampling, 50, optimize=True)]
    coef, status, px, intact = raw_decode(files)
    assert intact and status.tolist() == [0, 0, 0]
    for f, data in enumerate(files):
        assert np.array_equal(coef[f], ref(data)[0]) and np.array_equal(px[f], SC.pillow_decode(data)), f
    frames, st = video_in.decode_jpeg(files, DEV, with_status=True)
    assert frames.dtype == torch.uint8 and frames.is_cuda and st.tolist() == [0, 0, 0]
    assert torch.equal(frames.cpu(), torch.from_numpy(px.copy()).reshape(frames.shape))
    c2, s2, plan = video_in.decode_jpeg_coefficients(files, DEV)
    assert torch.equal(c2.cpu(), torch.from_numpy(coef.copy())) and s2.tolist() == [0, 0, 0] and plan.sampling == sampling


# ---- 2. damaged streams: bounded decodes of bad bytes ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(2), ids=lambda i: ("truncated", "unknown_code")[i])
@pytest.mark.parametrize("sampling", (R.S444, R.GRAY), ids=name_of)
def test_damaged_frame_is_reported_and_its_neighbours_are_not(sampling, case):
    from dino_tracker_amd import video_in
    name, bad = SC.damaged(sampling)[case]
    good = [SC.good_file(sampling, seed=1), SC.good_file(sampling, seed=2)]
    files = [good[0], bad, good[1]]
    coef, status, px, intact = raw_decode(files)
    assert intact and status.tolist() == [0, SC.STATUS[name], 0], status
    for f, data in ((0, good[0]), (2, good[1])):
        assert np.array_equal(coef[f], ref(data)[0]) and np.array_equal(px[f], SC.pillow_decode(data))
    try:
        want = SC.pillow_decode(bad)
    except Exception as e:   # noqa: BLE001   (what Pillow raises for the file, the fallback raises)
        with pytest.raises(type(e)):
            video_in.decode_jpeg(files, DEV)
        return
    frames, st = video_in.decode_jpeg(files, DEV, with_status=True)
    assert st.tolist() == [0, SC.STATUS[name], 0]
    assert np.array_equal(frames[1].cpu().numpy().reshape(want.shape), want)
    assert np.array_equal(frames[0].cpu().numpy().reshape(px[0].shape), px[0])


def test_refusals_write_nothing():
    from dino_tracker_amd import ops
    from dino_tracker_amd._lib import lib
    h = lib()
    whole, buf, start = guarded(1 << 16)
    p = buf.data_ptr()
    seg = np.array([[0, 0, 64, 0, 1]], dtype=np.int64)
    sp = seg.ctypes.data
    for bad in (-1, 4, 6):
        assert h.dtk_jpeg_decode_workspace_bytes_sampled(bad, 1, 8, 8) == 0
        assert h.dtk_jpeg_decode_coefficients_sampled(bad, p, 64, p, sp, 1, p, 1, 8, 8, p, p, None) == -1 and b"sampling" in h.dtk_last_error()
        assert h.dtk_jpeg_pixels_sampled(bad, p, p, 1, 8, 8, p, p, p, None) == -1 and b"sampling" in h.dtk_last_error()
    # 16 x 16: one MCU at 4:2:0, two at 4:2:2, four at 4:4:4 and gray -- the segment table is held to the sampling's count
    for S, mcus in ((R.S420, 1), (R.S422, 2), (R.S444, 4), (R.GRAY, 4)):
        assert h.dtk_jpeg_decode_workspace_bytes_sampled(S, 1, 16, 16) == -(-mcus * 64 * R.blocks_per_mcu(S) // 256) * 256
        for row in ([0, 0, 64, 0, mcus + 1], [0, 0, 64, mcus, 1], [0, 0, 64, 1, mcus], [1, 0, 64, 0, 1], [0, 1, 64, 0, 1]):
            bad = np.array([row], dtype=np.int64)
            assert h.dtk_jpeg_decode_coefficients_sampled(S, p, 64, p, bad.ctypes.data, 1, p, 1, 16, 16, p, p, None) == -1
            assert b"does not fit" in h.dtk_last_error()
        for F, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 65536)):
            assert h.dtk_jpeg_decode_workspace_bytes_sampled(S, F, H, W) == 0
            assert h.dtk_jpeg_pixels_sampled(S, p, p, F, H, W, p, p, p, None) == -1 and b"jpeg_pixels" in h.dtk_last_error()
    torch.cuda.synchronize()
    assert bool((whole == POISON).all())
    with pytest.raises(RuntimeError, match="sampling"):
        ops.jpeg_pixels(torch.zeros((1, 1, 6, 64), dtype=torch.int16, device=DEV), torch.zeros((1, 3, 64), dtype=torch.uint8, device=DEV),
                        8, 8, sampling=7)
    with pytest.raises(RuntimeError, match=r"huffman must be uint8 \[F, 1, 2, 272\]"):
        ops.jpeg_decode_coefficients(torch.zeros(8, dtype=torch.uint8, device=DEV), seg,
                                     torch.zeros((1, 3, 2, 272), dtype=torch.uint8, device=DEV), 8, 8, sampling=R.GRAY)


# ---- 3. the wiring -----------------------------------------------------------------------------------------------------------------
def _folder(path, files):
    path.mkdir()
    for t, data in enumerate(files):
        (path / f"{t:05d}.jpg").write_bytes(data)
    return str(path)


@pytest.mark.parametrize("sampling", SC.SAMPLINGS, ids=name_of)
def test_load_video_device_equals_host(sampling, tmp_path, monkeypatch):
    from dino_tracker_amd import video_in, video_io
    files = [SC.encode(SC.picture("noise", 48, 64, sampling, seed=s), sampling, 90) for s in range(3)]
    folder = _folder(tmp_path / "jpg", files)
    calls = []
    original = video_in.decode_planned
    monkeypatch.setattr(video_in, "decode_planned", lambda *a, **k: calls.append(1) or original(*a, **k))
    got = {}
    for mode, used in (("host", 0), ("device", 1)):
        monkeypatch.setenv("DTK_JPEG_DECODE", mode)
        calls.clear()
        got[mode] = video_io.load_video(folder, resize=(28, 42), device=DEV)
        assert len(calls) == used and got[mode].is_cuda, mode
        assert tuple(got[mode].shape) == (3, 1 if sampling == R.GRAY else 3, 28, 42)
    assert torch.equal(got["host"], got["device"])
    monkeypatch.setenv("DTK_JPEG_DECODE", "device")
    unresized = video_io.load_video(folder, device=DEV)
    want = np.stack([SC.pillow_decode(d).reshape(48, 64, -1) for d in files]).transpose(0, 3, 1, 2)
    assert torch.equal(unresized.cpu(), torch.from_numpy(want.copy()).float().div(255))
    # auto: the device decoder for exactly the samplings the measurements admitted (4:2:0 among them)
    monkeypatch.delenv("DTK_JPEG_DECODE")
    calls.clear()
    auto = video_io.load_video(folder, resize=(28, 42), device=DEV)
    assert torch.equal(auto, got["host"]) and len(calls) == (1 if sampling in video_io.JPEG_AUTO_SAMPLINGS else 0)
    assert R.S420 in video_io.JPEG_AUTO_SAMPLINGS


def test_a_folder_of_two_samplings_takes_the_host_path(tmp_path, monkeypatch):
    from dino_tracker_amd import video_in, video_io
    from dino_tracker_amd.train import load_video as host_load_video
    imgs = [SC.picture("noise", 48, 64, R.S444, seed=s) for s in range(3)]
    folder = _folder(tmp_path / "mixed", [SC.encode(imgs[0], R.S444, 90), SC.encode(imgs[1], R.S420, 90), SC.encode(imgs[2], R.S444, 90)])
    calls = []
    original = video_in.decode_planned
    monkeypatch.setattr(video_in, "decode_planned", lambda *a, **k: calls.append(1) or original(*a, **k))
    monkeypatch.setenv("DTK_JPEG_DECODE", "device")
    got = video_io.load_video(folder, resize=(28, 42), device=DEV)
    assert not calls and torch.equal(got.cpu(), host_load_video(folder, resize=(28, 42)))
    with pytest.raises(ValueError, match="file 1: sampling 4:2:0, file 0 is 4:4:4"):
        video_in.decode_jpeg(sorted(str(p) for p in (tmp_path / "mixed").iterdir()), DEV)


def test_adobe_transform_1_is_decoded(tmp_path):
    from dino_tracker_amd import video_in
    data = SC.encode(SC.picture("noise", 17, 33, R.S444), R.S444, 75)
    for keep_jfif in (True, False):
        adobe = SC.with_adobe(data, 1, keep_jfif)
        frames, st = video_in.decode_jpeg([adobe], DEV, fallback=False, with_status=True)
        assert st.tolist() == [0] and np.array_equal(frames[0].cpu().numpy(), SC.pillow_decode(adobe))
    with pytest.raises(ValueError, match="transform 0"):
        video_in.decode_jpeg([SC.with_adobe(data, 0)], DEV)
    with pytest.raises(ValueError, match="progressive"):
        video_in.decode_jpeg([SC.encode(SC.picture("noise", 17, 33, R.S444), R.S444, 75, progressive=True)], DEV)
