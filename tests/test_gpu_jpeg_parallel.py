"""GPU: the entropy stage that decodes ONE segment with many lanes (csrc/jpeg_parallel.hip, docs/JPEG_DECODE.md section 1b) through
ctypes on guarded buffers, the workspace included.  Coefficients and status must equal -- np.array_equal -- the plain-Python
restatement tests/jpeg_par_ref.py and the sequential entry point dtk_jpeg_decode_coefficients_sampled; pixels must equal Pillow's.
Nothing is compared against the code under test.

Shapes, chosen where this kernel can go wrong: segments shorter than one sub-stream and restart intervals of a few dozen bytes;
partial MCUs; the real 65 kB frame; a flat picture (about 190 blocks start in one sub-stream: the counts and the scan); quality-100
noise (blocks that span sub-streams, empty sub-streams, guesses that never merge); more than twice as many sub-streams as the
workgroup has lanes; unstuffed lengths of 0, 1 and 15 modulo 16; many stuffed FF 00 pairs; three table sets in one call; damaged
streams."""
import os

import numpy as np
import pytest
import torch

import jpeg_dec_cases as C
import jpeg_par_ref as P
import jpeg_sampling_cases as SC
import jpeg_sampling_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (5, 4), (9, 17), (17, 33), (31, 47), (40, 200)]
POISON = 0xA5
GUARD = 4096   # bytes
LANES = 1024   # of the kernel's workgroup
DEFAULT_L = 128
name_of = R.NAMES.get
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "horsejump_00000.jpg")

_REF = {}


def ref(data, L):
    """the sub-stream restatement's coefficients for one file, computed once and never modified (the entry states from the chain
    itself: the rounds are the CPU test's business)"""
    L = L or DEFAULT_L
    if (data, L) not in _REF:
        coef = P.coefficients(data, L, simulate=False)
        coef.setflags(write=False)
        _REF[data, L] = coef
    return _REF[data, L]


def guarded(nbytes):
    """(whole buffer filled with POISON, the 256-byte aligned view of `nbytes` between two guard bands, its start)"""
    whole = torch.full((GUARD + nbytes + 256 + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(whole.data_ptr() + GUARD)) % 256
    return whole, whole[start:start + nbytes], start


def bands_intact(whole, start, nbytes):
    return bool((whole[:start] == POISON).all()) and bool((whole[start + nbytes:] == POISON).all())


def entry_points(stream, segments, huffman, F, H, W, S, L, qtables=None):
    """both entropy entry points on the same bytes and tables, each into its own guarded buffers -> dict(par=(coef, status),
    seq=(coef, status), px=the pixel stage on the parallel coefficients (when qtables are given), intact)"""
    from dino_tracker_amd import ops
    from dino_tracker_amd._lib import lib
    h = lib()
    B = R.blocks_per_mcu(S)
    mh, mw = R.mcu_grid(H, W, S)
    mcus = mh * mw
    d_stream = torch.from_numpy(np.ascontiguousarray(stream)).to(DEV)
    seg = np.ascontiguousarray(segments, dtype=np.int64)
    d_seg, d_huff = torch.from_numpy(seg).to(DEV), torch.from_numpy(huffman).to(DEV)
    ws_bytes = h.dtk_jpeg_decode_parallel_workspace_bytes(S, d_stream.numel(), seg.shape[0], L)
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    sizes = (F * mcus * B * 128, 4 * F, ws_bytes, F * mcus * B * 128, 4 * F)
    bufs = [guarded(n) for n in sizes]
    coef_p, st_p, ws, coef_s, st_s = (b[1] for b in bufs)
    st = torch.cuda.current_stream().cuda_stream
    rc = h.dtk_jpeg_decode_coefficients_parallel(S, d_stream.data_ptr(), d_stream.numel(), d_seg.data_ptr(), seg.ctypes.data, seg.shape[0],
                                                 d_huff.data_ptr(), F, H, W, L, coef_p.data_ptr(), st_p.data_ptr(), ws.data_ptr(), st)
    assert rc == 0, h.dtk_last_error()
    rc = h.dtk_jpeg_decode_coefficients_sampled(S, d_stream.data_ptr(), d_stream.numel(), d_seg.data_ptr(), seg.ctypes.data, seg.shape[0],
                                                d_huff.data_ptr(), F, H, W, coef_s.data_ptr(), st_s.data_ptr(), st)
    assert rc == 0, h.dtk_last_error()
    px = None
    if qtables is not None:
        qt = torch.from_numpy(qtables).to(DEV)
        pw, pws, _ = guarded(ops.jpeg_decode_workspace_bytes(F, H, W, S))
        ow, out, ostart = guarded(F * H * W * (1 if S == R.GRAY else 3))
        rc = h.dtk_jpeg_pixels_sampled(S, coef_p.data_ptr(), qt.data_ptr(), F, H, W, out.data_ptr(), None, pws.data_ptr(), st)
        assert rc == 0, h.dtk_last_error()
        px = out.cpu().numpy().reshape((F, H, W) if S == R.GRAY else (F, H, W, 3))
    torch.cuda.synchronize()
    intact = all(bands_intact(b[0], b[2], n) for b, n in zip(bufs, sizes))
    as_coef = lambda t: t.cpu().numpy().view(np.int16).reshape(F, mcus, B, 64)   # noqa: E731
    as_status = lambda t: t.cpu().numpy().view(np.int32)                          # noqa: E731
    return dict(par=(as_coef(coef_p), as_status(st_p)), seq=(as_coef(coef_s), as_status(st_s)), px=px, intact=intact)


def decode_files(files, L):
    from dino_tracker_amd import video_in
    plan, why = video_in.plan_jpeg_sampled(files)
    assert plan is not None, why
    stream = np.frombuffer(b"".join(files), dtype=np.uint8).copy()
    return entry_points(stream, plan.segments, plan.huffman, plan.frames, plan.height, plan.width, plan.sampling, L, plan.qtables), plan


def check_files(files, L, tag=None):
    """the whole claim for valid files: status 0, coefficients = restatement = sequential entry point, pixels = Pillow, guards"""
    got, plan = decode_files(files, L)
    assert got["intact"], tag
    assert got["par"][1].tolist() == [0] * len(files) and got["seq"][1].tolist() == [0] * len(files), (tag, got["par"][1], got["seq"][1])
    assert np.array_equal(got["par"][0], got["seq"][0]), tag
    for f, data in enumerate(files):
        assert np.array_equal(got["par"][0][f], ref(data, L)), (tag, f)
        assert np.array_equal(got["px"][f], SC.pillow_decode(data)), (tag, f)
    return plan


def unstuffed_scan(data):
    return R.parse(data)["scan"].replace(b"\xff\x00", b"\xff")


# ---- 1. valid files ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sampling", SC.SAMPLINGS, ids=name_of)
def test_small_frames_every_sampling_and_variant(sampling, size):
    h, w = size
    for name, data in SC.variants(SC.picture("noise", h, w, sampling), sampling, 75):
        for L in (16, 64, 0):
            check_files([data], L, (size, name, L))


@pytest.mark.parametrize("L", (0, 32))
def test_the_real_frame(L):
    data = open(GOLDEN, "rb").read()
    plan = check_files([data], L)
    assert plan.segments.shape[0] == 1 and int(plan.segments[0, 2]) > 65000


@pytest.mark.parametrize("sampling", (R.S420, R.GRAY), ids=name_of)
def test_a_flat_picture_starts_many_blocks_per_substream(sampling):
    img = np.full((256, 256, 3), 90, dtype=np.uint8) if sampling != R.GRAY else np.full((256, 256), 90, dtype=np.uint8)
    data = SC.encode(img, sampling, 75)
    blocks = 1536 if sampling == R.S420 else 1024
    assert blocks / -(-len(unstuffed_scan(data)) // 128) > 100
    check_files([data], 0)
    check_files([data], 16)


@pytest.mark.parametrize("L", (16, 128))
def test_quality_100_noise_blocks_span_substreams(L):
    data = SC.encode(SC.picture("noise", 64, 64, R.S420), R.S420, 100)
    assert len(unstuffed_scan(data)) > 7000
    check_files([data], L)


def test_more_substreams_than_twice_the_lanes():
    data = SC.encode(SC.picture("noise", 160, 160, R.S444), R.S444, 100)
    assert -(-len(unstuffed_scan(data)) // 16) > 2 * LANES
    check_files([data], 16)


def test_unstuffed_lengths_around_a_multiple_of_16():
    found = {}
    for seed in range(400):
        data = SC.encode(SC.picture("noise", 16, 24, R.S420, seed=seed), R.S420, 75)
        found.setdefault(len(unstuffed_scan(data)) % 16, data)
        if all(r in found for r in (0, 1, 15)):
            break
    for r in (0, 1, 15):
        assert len(unstuffed_scan(found[r])) % 16 == r
        check_files([found[r]], 16, r)


def test_a_scan_with_many_stuffed_bytes():
    data = SC.encode(SC.picture("noise", 96, 96, R.S444), R.S444, 100)
    assert R.parse(data)["scan"].count(b"\xff\x00") >= 20
    check_files([data], 0)
    check_files([data], 16)


@pytest.mark.parametrize("sampling", SC.SAMPLINGS, ids=name_of)
def test_three_frames_three_table_sets_different_segment_counts(sampling):
    h, w = 33, 47
    files = [SC.encode(SC.picture("noise", h, w, sampling, seed=1), sampling, 90, optimize=True),
             SC.encode(SC.picture("ramp", h, w, sampling), sampling, 100, optimize=True, restart_marker_blocks=3),
             SC.encode(SC.picture("noise", h, w, sampling, seed=2), sampling, 50, optimize=True, restart_marker_blocks=2)]
    plan = check_files(files, 16)
    counts = [int((plan.segments[:, 0] == f).sum()) for f in range(3)]
    assert len(set(counts)) == 3 and len({plan.huffman[f].tobytes() for f in range(3)}) == 3
    check_files(files, 0)


# ---- 2. damaged streams: the sequential entry point's coefficients and status, whatever they are -------------------------------------
def damaged_streams(sampling):
    """(name, stream bytes, segment table) around one good single-segment file: the segment cut short, single-bit flips inside it,
    its tail overwritten with FF"""
    from dino_tracker_amd import video_in
    data = SC.good_file(sampling)
    plan, why = video_in.plan_jpeg_sampled([data])
    assert plan is not None and plan.segments.shape[0] == 1, why
    off, length = int(plan.segments[0, 1]), int(plan.segments[0, 2])
    base = np.frombuffer(data, dtype=np.uint8).copy()
    out = []
    for cut in (0, 1, 2, 15, 16, 17, length // 2, length - 1):
        seg = plan.segments.copy()
        seg[0, 2] = cut
        out.append((f"cut{cut}", base, seg))
    rng = np.random.default_rng(5)
    for _ in range(16):
        bit = int(rng.integers(0, 8 * length))
        v = base.copy()
        v[off + bit // 8] ^= 0x80 >> (bit % 8)
        out.append((f"flip{bit}", v, plan.segments))
    for tail in (1, 17, length):
        v = base.copy()
        v[off + length - tail:off + length] = 0xFF
        out.append((f"ff{tail}", v, plan.segments))
    return plan, out


@pytest.mark.parametrize("sampling", SC.SAMPLINGS, ids=name_of)
def test_damaged_streams_equal_the_sequential_entry_point(sampling):
    plan, cases = damaged_streams(sampling)
    statuses = set()
    for name, stream, seg in cases:
        for L in (16, 0):
            got = entry_points(stream, seg, plan.huffman, 1, plan.height, plan.width, sampling, L)
            assert got["intact"], (name, L)
            assert got["par"][1].tolist() == got["seq"][1].tolist(), (name, L, got["par"][1], got["seq"][1])
            assert np.array_equal(got["par"][0], got["seq"][0]), (name, L)
            statuses.add(int(got["seq"][1][0]))
    assert len(statuses - {0}) >= 2, statuses       # the copies are damaged in more than one way


@pytest.mark.parametrize("case", range(2), ids=lambda i: ("truncated", "unknown_code")[i])
def test_a_damaged_frame_between_two_good_ones_falls_back_to_pillow(case):
    from dino_tracker_amd import video_in
    name, bad = SC.damaged(R.S444)[case]
    good = [SC.good_file(R.S444, seed=1), SC.good_file(R.S444, seed=2)]
    files = [good[0], bad, good[1]]
    got, _ = decode_files(files, 16)
    assert got["intact"] and got["par"][1].tolist() == [0, SC.STATUS[name], 0] == got["seq"][1].tolist()
    assert np.array_equal(got["par"][0], got["seq"][0])
    for f in (0, 2):
        assert np.array_equal(got["par"][0][f], ref(files[f], 16)) and np.array_equal(got["px"][f], SC.pillow_decode(files[f]))
    try:
        want = SC.pillow_decode(bad)
    except Exception as e:   # noqa: BLE001   (what Pillow raises for the file, the fallback raises)
        with pytest.raises(type(e)):
            video_in.decode_jpeg(files, DEV, entropy="parallel", subseq_bytes=16)
        return
    frames, st = video_in.decode_jpeg(files, DEV, with_status=True, entropy="parallel", subseq_bytes=16)
    assert st.tolist() == [0, SC.STATUS[name], 0]
    assert np.array_equal(frames[1].cpu().numpy(), want)
    for f in (0, 2):
        assert np.array_equal(frames[f].cpu().numpy(), SC.pillow_decode(files[f])), f


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    from dino_tracker_amd import ops
    from dino_tracker_amd._lib import lib
    h = lib()
    whole, buf, start = guarded(1 << 16)
    p = buf.data_ptr()
    seg = np.array([[0, 0, 64, 0, 1]], dtype=np.int64)
    sp = seg.ctypes.data

    def call(S=R.S420, stream_bytes=64, segs=sp, n=1, L=0, ws=p):
        return h.dtk_jpeg_decode_coefficients_parallel(S, p, stream_bytes, p, segs, n, p, 1, 8, 8, L, p, p, ws, None)

    for L in (-16, 4, 12, 18, 1028, 2048):
        assert h.dtk_jpeg_decode_parallel_workspace_bytes(R.S420, 64, 1, L) == 0
        assert call(L=L) == -1 and b"subseq_bytes" in h.dtk_last_error()
    for L in (0, 16, 20, 128, 1024):
        assert h.dtk_jpeg_decode_parallel_workspace_bytes(R.S420, 64, 1, L) > 64
    for S in (-1, 4):
        assert h.dtk_jpeg_decode_parallel_workspace_bytes(S, 64, 1, 0) == 0
        assert call(S=S) == -1 and b"sampling" in h.dtk_last_error()
    assert h.dtk_jpeg_decode_parallel_workspace_bytes(R.S420, 0, 1, 0) == 0 and h.dtk_jpeg_decode_parallel_workspace_bytes(R.S420, 64, 0, 0) == 0
    for row in ([0, 1, 64, 0, 1], [0, -1, 8, 0, 1], [0, 0, 65, 0, 1], [1, 0, 64, 0, 1], [0, 0, 64, 1, 1], [0, 0, 64, 0, 2]):
        bad = np.array([row], dtype=np.int64)
        assert call(segs=bad.ctypes.data) == -1 and b"does not fit" in h.dtk_last_error()
    overlap = np.array([[0, 0, 40, 0, 1], [0, 32, 32, 0, 1]], dtype=np.int64)     # rows whose bytes overlap: no place in the workspace
    assert call(segs=overlap.ctypes.data, n=2) == -1 and b"inside or before" in h.dtk_last_error()
    assert call(ws=None) == -1 and b"null pointer" in h.dtk_last_error()
    torch.cuda.synchronize()
    assert bool((whole == POISON).all())
    with pytest.raises(RuntimeError, match="subseq_bytes"):
        ops.jpeg_decode_coefficients_parallel(torch.zeros(8, dtype=torch.uint8, device=DEV), seg,
                                              torch.zeros((1, 3, 2, 272), dtype=torch.uint8, device=DEV), 8, 8, subseq_bytes=10)


def test_device_copy_of_the_segment_table_is_checked_too():
    from dino_tracker_amd import video_in
    from dino_tracker_amd._lib import lib
    data = SC.good_file(R.S444)
    plan, _ = video_in.plan_jpeg_sampled([data])
    stream = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(DEV)
    lying = plan.segments.copy()
    lying[0, 2] = len(data) + 1000          # the device copy claims bytes beyond the stream
    mh, mw = R.mcu_grid(plan.height, plan.width, R.S444)
    whole, coef, start = guarded(mh * mw * 3 * 128)
    n = lib().dtk_jpeg_decode_parallel_workspace_bytes(R.S444, len(data), 1, 0)
    wws, ws, wstart = guarded(n)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    d_lying, d_huff = torch.from_numpy(lying).to(DEV), torch.from_numpy(plan.huffman).to(DEV)   # alive until the kernel has run
    rc = lib().dtk_jpeg_decode_coefficients_parallel(R.S444, stream.data_ptr(), len(data), d_lying.data_ptr(), plan.segments.ctypes.data,
                                                     1, d_huff.data_ptr(), 1, plan.height, plan.width, 0, coef.data_ptr(),
                                                     status.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == [C.S_SEGMENT] and bool((whole == POISON).all()) and bool((wws == POISON).all())


# ---- 4. the wiring -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", SC.SAMPLINGS, ids=name_of)
def test_decode_jpeg_parallel_equals_pillow(sampling):
    from dino_tracker_amd import video_in
    files = [SC.encode(SC.picture("noise", 40, 56, sampling, seed=s), sampling, 90) for s in range(2)]
    for L in (0, 32):
        frames, st = video_in.decode_jpeg(files, DEV, fallback=False, with_status=True, entropy="parallel", subseq_bytes=L)
        assert st.tolist() == [0, 0]
        for f, data in enumerate(files):
            assert np.array_equal(frames[f].cpu().numpy().reshape(SC.pillow_decode(data).shape), SC.pillow_decode(data))
    coef, status, plan = video_in.decode_jpeg_coefficients(files, DEV, entropy="parallel")
    want, _, _ = video_in.decode_jpeg_coefficients(files, DEV, entropy="sequential")
    assert np.array_equal(coef.cpu().numpy()[0], ref(files[0], 0)) and torch.equal(coef, want) and status.tolist() == [0, 0]
    with pytest.raises(ValueError, match="entropy"):
        video_in.decode_jpeg(files, DEV, entropy="both")


def test_load_video_with_the_environment_variable(tmp_path, monkeypatch):
    from dino_tracker_amd import ops, video_io
    files = [SC.encode(SC.picture("noise", 48, 64, R.S420, seed=s), R.S420, 90) for s in range(5)]
    folder = tmp_path / "jpg"
    folder.mkdir()
    for t, data in enumerate(files):
        (folder / f"{t:05d}.jpg").write_bytes(data)
    calls = []
    original = ops.jpeg_decode_coefficients_parallel
    monkeypatch.setattr(ops, "jpeg_decode_coefficients_parallel", lambda *a, **k: calls.append(1) or original(*a, **k))
    monkeypatch.delenv("DTK_JPEG_ENTROPY", raising=False)
    default = video_io.load_video(str(folder), resize=(28, 42), device=DEV)
    assert not calls
    monkeypatch.setenv("DTK_JPEG_ENTROPY", "parallel")
    parallel = video_io.load_video(str(folder), resize=(28, 42), device=DEV)
    assert len(calls) == 1 and torch.equal(parallel, default)
    monkeypatch.setenv("DTK_JPEG_ENTROPY", "fast")
    with pytest.raises(ValueError, match="DTK_JPEG_ENTROPY"):
        video_io.load_video(str(folder), resize=(28, 42), device=DEV)
