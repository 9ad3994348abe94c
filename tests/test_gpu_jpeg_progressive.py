"""GPU: the device decoder of PROGRESSIVE JPEG files (csrc/jpeg_progressive.hip, csrc/jpeg_entropy.h, dino_tracker_amd/video_in.py)
against the plain-Python restatement of docs/JPEG_DECODE.md "Progressive files" (tests/jpeg_prog_ref.py) and against Pillow's decoder
-- never against the code under test.  Everything is an equality: the arithmetic is integer.  The restatement's own agreement with
the baseline coefficients and with Pillow over many more files is the CPU file's business
(tests/test_jpeg_progressive_reference.py).

Sizes (H x W): one pixel; 5 x 4; 9 x 17; 17 x 33 and 33 x 15 (at 4:2:0 and 4:2:2 the real block grid of a one-component scan is
smaller than the MCU padding); 31 x 47; 40 x 200 (more than one group of 32 blocks per segment, more than one restart interval)."""
import numpy as np
import pytest
import torch

import jpeg_prog_cases as C
import jpeg_prog_ref as P
import jpeg_sampling_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (5, 4), (9, 17), (17, 33), (31, 47), (33, 15), (40, 200)]
POISON = 0xA5
GUARD = 4096   # bytes
STAGING = 4096   # csrc/jpeg_progressive.hip EBUF: the unstuffed bytes of a segment staged at a time

_REF = {}


def ref(data):
    """the restatement's coefficients of one file, computed once and never modified"""
    if data not in _REF:
        coef = P.coefficients(data)
        coef.setflags(write=False)
        _REF[data] = coef
    return _REF[data]


def guarded(nbytes):
    """(whole buffer filled with POISON, the 256-byte aligned view of `nbytes` between two guard bands, its start)"""
    whole = torch.full((GUARD + nbytes + 256 + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(whole.data_ptr() + GUARD)) % 256
    return whole, whole[start:start + nbytes], start


def bands_intact(whole, start, nbytes):
    return bool((whole[:start] == POISON).all()) and bool((whole[start + nbytes:] == POISON).all())


def raw_decode(files, device_rows=None):
    """the entry point through ctypes on guarded buffers, then the pixel stage -> (coef int16 [F, MCUs, B, 64], status [F], pixels uint8
    [F, H, W, 3] or [F, H, W], every guard band intact, the plan).  device_rows: what the DEVICE copy of the table holds instead."""
    from dino_tracker_amd import ops, video_in
    from dino_tracker_amd._lib import lib
    plan, why = video_in.plan_jpeg_progressive(files)
    assert plan is not None, why
    F, H, W, S = plan.frames, plan.height, plan.width, plan.sampling
    B = R.blocks_per_mcu(S)
    mcus = int(np.prod(R.mcu_grid(H, W, S)))
    stream = torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy()).to(DEV)
    seg = torch.from_numpy(plan.segments if device_rows is None else device_rows).to(DEV)
    tables, qt = torch.from_numpy(plan.tables).to(DEV), torch.from_numpy(plan.qtables).to(DEV)
    sizes = (F * mcus * B * 128, 4 * F, F * H * W * (1 if S == R.GRAY else 3), ops.jpeg_decode_workspace_bytes(F, H, W, S))
    bufs = [guarded(n) for n in sizes]
    coef, status, out, ws = (b[1] for b in bufs)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib().dtk_jpeg_decode_progressive(S, stream.data_ptr(), stream.numel(), seg.data_ptr(), plan.segments.ctypes.data,
                                           plan.segments.shape[0], tables.data_ptr(), plan.tables.shape[0], F, H, W, coef.data_ptr(),
                                           status.data_ptr(), st)
    assert rc == 0, lib().dtk_last_error()
    rc = lib().dtk_jpeg_pixels_sampled(S, coef.data_ptr(), qt.data_ptr(), F, H, W, out.data_ptr(), status.data_ptr(), ws.data_ptr(), st)
    assert rc == 0, lib().dtk_last_error()
    torch.cuda.synchronize()
    intact = all(bands_intact(b[0], b[2], n) for b, n in zip(bufs, sizes))
    return (coef.cpu().numpy().view(np.int16).reshape(F, mcus, B, 64), status.cpu().numpy().view(np.int32),
            out.cpu().numpy().reshape((F, H, W) if S == R.GRAY else (F, H, W, 3)), intact, plan)


# ---- 1. coefficients and pixels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_files_equal_the_restatement_and_pillow(size):
    h, w = size
    for sampling in C.SAMPLINGS:
        for restart, _ in C.RESTARTS:
            for kind, q in (("noise", 75), ("ramp", 100)):
                _, data = C.pair(kind, h, w, sampling, q, restart)
                what = (size, R.NAMES[sampling], restart, kind, q)
                coef, status, px, intact, _ = raw_decode([data])
                assert intact and status.tolist() == [0], (what, status)
                assert np.array_equal(coef[0], ref(data)), what
                assert np.array_equal(px[0], C.pillow_decode(data)), what


def test_long_end_of_band_runs():
    """the flat 1024 x 1024 gray file: 16 384 blocks in 4.4 kB, end-of-band runs of category 14 in first and refinement scans"""
    data = C.flat_file()
    coef, status, px, intact, _ = raw_decode([data])
    assert intact and status.tolist() == [0]
    assert np.array_equal(coef[0], ref(data)) and np.array_equal(px[0], C.pillow_decode(data))


def test_a_segment_of_several_staging_buffers():
    """noise at quality 100: the first scan of the luma band 6-63 is one segment many refills long"""
    data = C.pair("noise", 128, 192, R.GRAY, 100)[1]
    coef, status, px, intact, plan = raw_decode([data])
    assert int(plan.segments[:, 2].max()) >= 3 * STAGING, plan.segments[:, 2]
    assert intact and status.tolist() == [0]
    assert np.array_equal(coef[0], ref(data)) and np.array_equal(px[0], C.pillow_decode(data))


@pytest.mark.parametrize("sampling", C.SAMPLINGS, ids=lambda s: R.NAMES[s])
def test_three_frames_with_their_own_tables(sampling):
    """three pictures, three qualities, three restart settings: three sets of tables and segment layouts in ONE call"""
    from dino_tracker_amd import video_in
    h, w = 33, 50
    files = [C.pair("noise", h, w, sampling, 90, "blocks3", seed=1)[1], C.pair("ramp", h, w, sampling, 100)[1],
             C.pair("noise", h, w, sampling, 50, "rows1", seed=2)[1]]
    coef, status, px, intact, plan = raw_decode(files)
    assert intact and status.tolist() == [0, 0, 0] and plan.tables.shape[0] > 10
    for f, data in enumerate(files):
        assert np.array_equal(coef[f], ref(data)), f
        assert np.array_equal(px[f], C.pillow_decode(data)), f
    # the public entry points: the same frames, from bytes
    frames, st = video_in.decode_jpeg_progressive(files, DEV, with_status=True)
    want = torch.from_numpy(px.copy())
    assert frames.dtype == torch.uint8 and frames.is_cuda and st.tolist() == [0, 0, 0]
    assert torch.equal(frames.cpu(), want[..., None] if sampling == R.GRAY else want)
    c2, s2, plan2 = video_in.decode_jpeg_progressive_coefficients(files, DEV)
    assert torch.equal(c2.cpu(), torch.from_numpy(coef.copy())) and s2.tolist() == [0, 0, 0] and plan2.frames == 3


def test_the_real_frame():
    """854 x 480 re-encoded as a progressive file: ten scans without restart markers, every one a single long segment"""
    from dino_tracker_amd import video_in
    data = C.real_frame()
    frames, status = video_in.decode_jpeg_progressive([data], DEV, fallback=False, with_status=True)
    assert status.tolist() == [0]
    assert torch.equal(frames[0].cpu(), torch.from_numpy(C.pillow_decode(data)))
    coef, _, _ = video_in.decode_jpeg_progressive_coefficients([data], DEV)
    assert np.array_equal(coef[0].cpu().numpy(), ref(data))


# ---- 2. damaged streams, lying tables, refusals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(2), ids=lambda i: ("truncated", "unknown_code")[i])
def test_damaged_frame_is_reported_and_its_neighbours_are_not(case):
    from dino_tracker_amd import video_in
    name, bad = C.damaged()[case]
    good = [C.good_file(seed=1), C.good_file(seed=2)]
    files = [good[0], bad, good[1]]
    coef, status, px, intact, _ = raw_decode(files)
    assert intact and status.tolist() == [0, C.STATUS[name], 0], status
    for f, data in ((0, good[0]), (2, good[1])):
        assert np.array_equal(coef[f], ref(data)) and np.array_equal(px[f], C.pillow_decode(data))
    frames, st = video_in.decode_jpeg_progressive(files, DEV, with_status=True)
    assert st.tolist() == [0, C.STATUS[name], 0]
    for f, data in enumerate(files):                       # the damaged frame's slot holds what Pillow makes of it
        assert np.array_equal(frames[f].cpu().numpy(), C.pillow_decode(data)), f
    raw = video_in.decode_jpeg_progressive(files, DEV, fallback=False)
    assert torch.equal(raw[0], frames[0]) and torch.equal(raw[2], frames[2])


def test_device_copy_of_the_segment_table_is_checked_too():
    """the kernel repeats the row check on ITS copy of the table: a row that does not fit decodes nothing"""
    data = C.good_file()
    from dino_tracker_amd import video_in
    plan, _ = video_in.plan_jpeg_progressive([data])
    rows = plan.segments
    for field, value in ((1, -8), (2, len(data) + 1000), (3, 7), (5, 64), (7, 14), (8, 3), (9, 1 << 20), (10, 1 << 20)):
        lying = rows.copy()
        lying[:, field] = value                             # every row fails: nothing but the zeroing is written
        coef, status, _, intact, _ = raw_decode([data], device_rows=lying)
        assert intact and status.tolist() == [C.S_SEGMENT] and not coef.any(), (field, status)
    lying = rows.copy()
    lying[:, 11:14] = plan.tables.shape[0]                  # tables beyond the array: every row that uses one fails
    coef, status, _, intact, _ = raw_decode([data], device_rows=lying)
    assert intact and status.tolist() == [C.S_SEGMENT] and not coef[..., 1:].any()
    lying = rows.copy()
    lying[0, 0] = 1                                         # a frame beyond F has no status word to report to: it stays silent
    coef, status, _, intact, _ = raw_decode([data], device_rows=lying)
    assert intact and np.array_equal(coef[0][..., 0], ref(data)[..., 0] & 1)   # row 0 is the interleaved DC scan: only the DC
    #                                                                            refinement's bit is there


def test_refusals_write_nothing():
    from dino_tracker_amd import ops, video_in
    from dino_tracker_amd._lib import lib
    h = lib()
    whole, buf, start = guarded(1 << 16)
    p = buf.data_ptr()
    good = [0, 0, 64, 0, 1, 5, 0, 2, 0, 0, 4, 1, 0, 0]     # 16 x 16 at 4:2:0: one MCU, four luma blocks
    seg = np.array([good], dtype=np.int64)
    sp = seg.ctypes.data
    call = h.dtk_jpeg_decode_progressive
    for S, F, H, W in ((0, 0, 16, 16), (0, 1, 0, 16), (0, 1, 16, 0), (0, 1, 65536, 16), (0, 1, 16, 65536), (0, -1, 16, 16), (4, 1, 16, 16),
                       (-1, 1, 16, 16)):
        assert call(S, p, 64, p, sp, 1, p, 2, F, H, W, p, p, None) == -1 and b"jpeg_decode_progressive" in h.dtk_last_error()
    for hole in (1, 3, 4, 6, 11, 12):
        args = [0, p, 64, p, sp, 1, p, 2, 1, 16, 16, p, p, None]
        args[hole] = None
        assert call(*args) == -1 and b"null pointer" in h.dtk_last_error()
    assert call(0, p, 0, p, sp, 1, p, 2, 1, 16, 16, p, p, None) == -1
    assert call(0, p, 64, p, sp, 0, p, 2, 1, 16, 16, p, p, None) == -1
    assert call(0, p, 64, p, sp, 1, p, 0, 1, 16, 16, p, p, None) == -1
    for field, value in ((0, 1), (0, -1), (1, 1), (1, -1), (2, 65), (2, -1), (3, -1), (3, 256), (4, 0), (4, 6), (5, 64), (6, 1), (7, 14),
                         (7, -1), (8, 3), (8, -1), (9, 1), (9, -1), (10, 5), (10, 0), (11, 2), (11, -1)):
        bad = seg.copy()
        bad[0, field] = value
        assert call(0, p, 64, p, bad.ctypes.data, 1, p, 2, 1, 16, 16, p, p, None) == -1, (field, value)
        assert b"does not fit" in h.dtk_last_error()
    two = np.array([good, good], dtype=np.int64)
    two[0, 3] = 1                                           # the rows are not ordered by level
    assert call(0, p, 64, p, two.ctypes.data, 2, p, 2, 1, 16, 16, p, p, None) == -1 and b"level" in h.dtk_last_error()
    torch.cuda.synchronize()
    assert bool((whole == POISON).all())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video_in.decode_jpeg_progressive([C.good_file()], "cpu")
    with pytest.raises(ValueError, match="not progressive"):
        video_in.decode_jpeg_progressive([C.pair("noise", 16, 16, R.S420, 90)[0]], DEV)
    with pytest.raises(ValueError, match="incomplete progression"):
        video_in.decode_jpeg_progressive([C.cut_after_scans(C.good_file(), 5)], DEV)
    with pytest.raises(ValueError, match="progressive"):
        video_in.decode_jpeg([C.good_file()], DEV)          # the baseline entry point keeps refusing
    stream = torch.zeros(8, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="segments"):
        ops.jpeg_decode_progressive(stream, np.zeros((1, 5), np.int64), torch.zeros((1, 272), dtype=torch.uint8, device=DEV), 1, 8, 8)
    with pytest.raises(RuntimeError, match="tables"):
        ops.jpeg_decode_progressive(stream, np.zeros((1, 14), np.int64), torch.zeros((1, 2, 272), dtype=torch.uint8, device=DEV), 1, 8, 8)
    with pytest.raises(RuntimeError, match="does not fit"):
        ops.jpeg_decode_progressive(stream, np.array([good], np.int64), torch.zeros((2, 272), dtype=torch.uint8, device=DEV), 1, 16, 16)


# ---- 3. the wiring ----------------------------------------------------------------------------------------------------------------------------
def _folder(path, files, suffix=".jpg"):
    path.mkdir()
    for t, data in enumerate(files):
        (path / f"{t:05d}{suffix}").write_bytes(data)
    return str(path)


def test_load_video_takes_the_progressive_decoder_only_when_asked(tmp_path, monkeypatch):
    from dino_tracker_amd import video_in, video_io
    from dino_tracker_amd.train import load_video as host_load_video
    pairs = [C.pair("noise", 48, 64, R.S420, 90, seed=s) for s in range(3)]
    folder = _folder(tmp_path / "prog", [p[1] for p in pairs])
    want = host_load_video(folder, resize=(28, 42))
    calls, baseline_calls = [], []
    original, baseline = video_in.decode_planned_progressive, video_in.decode_planned
    monkeypatch.setattr(video_in, "decode_planned_progressive", lambda *a, **k: calls.append(1) or original(*a, **k))
    monkeypatch.setattr(video_in, "decode_planned", lambda *a, **k: baseline_calls.append(1) or baseline(*a, **k))
    for mode, used in ((None, 0), ("auto", 0), ("host", 0), ("device", 1)):
        calls.clear()
        if mode is None:
            monkeypatch.delenv("DTK_JPEG_DECODE", raising=False)
        else:
            monkeypatch.setenv("DTK_JPEG_DECODE", mode)
        got = video_io.load_video(folder, resize=(28, 42), device=DEV)
        assert len(calls) == used and not baseline_calls and got.is_cuda and torch.equal(got.cpu(), want), mode
    # still under `device`: without a resize, and the first two frames only
    assert torch.equal(video_io.load_video(folder, device=DEV, num_frames=2).cpu(), host_load_video(folder)[:2])
    assert len(calls) == 2
    # a folder that mixes progressive and baseline files goes to the host; so does one with an incomplete file
    calls.clear()
    mixed = _folder(tmp_path / "mixed", [pairs[0][1], pairs[1][0], pairs[2][1]])
    assert torch.equal(video_io.load_video(mixed, resize=(28, 42), device=DEV).cpu(), host_load_video(mixed, resize=(28, 42)))
    cut = _folder(tmp_path / "cut", [pairs[0][1], C.cut_after_scans(pairs[1][1], 5)])
    assert torch.equal(video_io.load_video(cut, device=DEV).cpu(), host_load_video(cut))
    assert not calls and not baseline_calls
    # gray progressive files: [T, 1, h, w]; the host path for those is video_io's own (Pillow into a pinned buffer, the device resize)
    gray = _folder(tmp_path / "gray", [C.pair("noise", 48, 64, R.GRAY, 90, seed=s)[1] for s in range(2)])
    got = video_io.load_video(gray, resize=(28, 42), device=DEV)
    monkeypatch.setenv("DTK_JPEG_DECODE", "host")
    assert len(calls) == 1 and tuple(got.shape) == (2, 1, 28, 42) and torch.equal(got, video_io.load_video(gray, resize=(28, 42), device=DEV))
    monkeypatch.setenv("DTK_JPEG_DECODE", "device")
    # a damaged frame in the folder: Pillow's pixels in its slot, as the host path has them
    bad = _folder(tmp_path / "bad", [C.good_file(seed=1), C.damaged()[0][1], C.good_file(seed=2)])
    assert torch.equal(video_io.load_video(bad, device=DEV).cpu(), host_load_video(bad))
    assert len(calls) == 2


def test_the_real_frame_through_load_video(tmp_path, monkeypatch):
    from dino_tracker_amd import video_io
    from dino_tracker_amd.train import load_video as host_load_video
    folder = _folder(tmp_path / "real", [C.real_frame()] * 2)
    monkeypatch.setenv("DTK_JPEG_DECODE", "device")
    assert torch.equal(video_io.load_video(folder, resize=(120, 214), device=DEV).cpu(), host_load_video(folder, resize=(120, 214)))
