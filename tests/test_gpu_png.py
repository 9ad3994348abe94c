"""GPU: the device PNG decoder (csrc/inflate.hip, csrc/inflate_core.h, dino_tracker_amd/png_in.py) against zlib.decompress, the
original arrays, Pillow and -- for statuses -- the plain-Python restatement (tests/png_ref.py); never against the code under test.
Everything is an equality: the format is lossless.  Output and status sit in poisoned buffers between guard bands.

Unfilter sizes (H x W): 1 x 1; 1 x 5 (no row above); 5 x 1 (no left neighbour); 3 x 67 (longer than a wave); 65 x 33 (crosses a
64-row block); 130 x 7 (two crossings); 32 x 854 (the pipeline's row length)."""
import io
import random
import struct
import zlib

import numpy as np
import pytest
import torch

import png_cases as C
import png_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xA5
GUARD = 4096
SIZES = [(1, 1), (1, 5), (5, 1), (3, 67), (65, 33), (130, 7), (32, 854)]
E_INVALID = -1


def guarded(nbytes):
    """(whole buffer filled with POISON, the 256-byte aligned view of `nbytes` between two guard bands, its start)"""
    whole = torch.full((GUARD + nbytes + 256 + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(whole.data_ptr() + GUARD)) % 256
    return whole, whole[start:start + nbytes], start


def bands_intact(whole, start, nbytes):
    return bool((whole[:start] == POISON).all()) and bool((whole[start + nbytes:] == POISON).all())


def run_inflate(jobs, wrapper=1, seed=None, adler=True, gap=0):
    """jobs: [(stream bytes, expected output bytes)].  The streams lie one after the other in the input; their output ranges are
    laid out in a shuffled order (seed) with `gap` poisoned bytes between them.  -> ([output bytes], [status], intact): `intact`
    covers the guard bands of output and status and the gaps."""
    from dino_tracker_amd._lib import lib
    order = list(range(len(jobs)))
    if seed is not None:
        random.Random(seed).shuffle(order)
    table = np.zeros((len(jobs), 4), dtype=np.int64)
    at = 0
    for k in order:
        table[k, 2], table[k, 3] = at, jobs[k][1]
        at += jobs[k][1] + gap
    total = max(1, at)
    blob = b"".join(s for s, _ in jobs) or b"\x00"
    table[:, 0] = np.concatenate(([0], np.cumsum([len(s) for s, _ in jobs])))[:-1]
    table[:, 1] = [len(s) for s, _ in jobs]
    src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(DEV)
    tab = torch.from_numpy(table).to(DEV)
    (ow, out, ostart), (sw, status, sstart) = guarded(total), guarded(4 * len(jobs))
    st = torch.cuda.current_stream().cuda_stream
    rc = lib().dtk_inflate(src.data_ptr(), src.numel(), tab.data_ptr(), table.ctypes.data, len(jobs), wrapper, out.data_ptr(), total,
                           status.data_ptr(), st)
    assert rc == 0, lib().dtk_last_error()
    if adler and wrapper:
        rc = lib().dtk_adler32(src.data_ptr(), src.numel(), tab.data_ptr(), table.ctypes.data, len(jobs), out.data_ptr(), total,
                               status.data_ptr(), st)
        assert rc == 0, lib().dtk_last_error()
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    intact = bands_intact(ow, ostart, total) and bands_intact(sw, sstart, 4 * len(jobs))
    for k in range(len(jobs)):
        o, n = int(table[k, 2]), int(table[k, 3])
        intact = intact and bool((host[o + n:o + n + gap] == POISON).all()) if gap and o + n + gap <= total else intact
    outs = [host[int(table[k, 2]):int(table[k, 2]) + int(table[k, 3])].tobytes() for k in range(len(jobs))]
    return outs, status.cpu().numpy().view(np.int32).tolist(), intact


# ---- 1. inflate ------------------------------------------------------------------------------------------------------------------
def test_every_valid_case_alone():
    for name, stream, data in C.cases():
        assert zlib.decompress(stream) == data
        outs, status, intact = run_inflate([(stream, len(data))])
        assert intact and status == [0] and outs[0] == data, (name, status)


def test_all_valid_cases_in_one_call_with_shuffled_outputs():
    cases = C.cases()
    outs, status, intact = run_inflate([(s, len(d)) for _, s, d in cases], seed=4, gap=7)
    assert intact and status == [0] * len(cases), status
    for (name, _, data), got in zip(cases, outs):
        assert got == data, name


def test_raw_mode_on_the_same_bodies():
    cases = C.cases()
    outs, status, intact = run_inflate([(s[2:-4], len(d)) for _, s, d in cases], wrapper=0, seed=5, gap=3)
    assert intact and status == [0] * len(cases), status
    for (name, _, data), got in zip(cases, outs):
        assert got == data, name


def test_damaged_cases_mixed_with_valid_streams():
    valid = {name: (s, d) for name, s, d in C.cases()}
    good = [valid[n] for n in ("default_dynamic", "hand_length3_distance1", "z_fixed")]
    jobs, want, bodies = [], [], []
    for k, (name, stream, expected, status, _) in enumerate(C.damaged()):
        body, ref_status, _ = R.inflate(stream, expected)
        assert ref_status == status, name
        jobs.append((stream, expected)), want.append(status), bodies.append(body)
        s, d = good[k % len(good)]
        jobs.append((s, len(d))), want.append(0), bodies.append(d)
    outs, status, intact = run_inflate(jobs, seed=6, gap=5)
    assert intact and status == want, list(zip([n for n, *_ in C.damaged()], status[::2], want[::2]))
    for k, (got, body) in enumerate(zip(outs, bodies)):
        assert got == body, (k, C.damaged()[k // 2][0])     # decoded up to the fault, zeros after it; neighbours untouched
    # the fault point: a truncated stream keeps a prefix of what the whole stream holds, the rest is zero
    names = [n for n, *_ in C.damaged()]
    cut, whole = names.index([n for n in names if n.startswith("truncated_to_")][5]), names.index("output_one_byte_longer")
    expected, full, got = C.damaged()[cut][2], zlib.decompress(C.damaged()[whole][1]), outs[2 * cut]
    keep = len(got.rstrip(b"\x00"))
    assert 0 < keep < expected and got[:keep] == full[:keep] and got[keep:] == bytes(expected - keep)


def test_adler32_alone():
    """on known bytes, without dtk_inflate: right and wrong trailers, an odd length, a status that is already set"""
    from dino_tracker_amd._lib import lib
    datas = [C.random_bytes(n, 20 + n % 7) for n in (1, 15, 4096, 4097, 70001, 300000)] + [bytes([255]) * 200000]
    trailers = [struct.pack(">I", zlib.adler32(d)) for d in datas]
    trailers[2] = bytes([trailers[2][0] ^ 0x80]) + trailers[2][1:]
    trailers[4] = trailers[4][:3] + bytes([trailers[4][3] ^ 1])
    table = np.zeros((len(datas), 4), dtype=np.int64)
    table[:, 0] = 8 * np.arange(len(datas))
    table[:, 1] = 8
    table[:, 2] = np.concatenate(([0], np.cumsum([len(d) for d in datas])))[:-1]
    table[:, 3] = [len(d) for d in datas]
    src = torch.from_numpy(np.frombuffer(b"".join(b"\x78\x9c\x03\x00" + t for t in trailers), dtype=np.uint8).copy()).to(DEV)
    out = torch.from_numpy(np.frombuffer(b"".join(datas), dtype=np.uint8).copy()).to(DEV)
    tab = torch.from_numpy(table).to(DEV)
    sw, status, sstart = guarded(4 * len(datas))
    status.view(torch.int32).zero_()
    status.view(torch.int32)[5] = R.S_CODE
    rc = lib().dtk_adler32(src.data_ptr(), src.numel(), tab.data_ptr(), table.ctypes.data, len(datas), out.data_ptr(), out.numel(),
                           status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib().dtk_last_error()
    torch.cuda.synchronize()
    assert status.cpu().numpy().view(np.int32).tolist() == [0, 0, R.S_ADLER, 0, R.S_ADLER, R.S_CODE, 0]
    assert bands_intact(sw, sstart, 4 * len(datas))


# ---- 2. the row filters ------------------------------------------------------------------------------------------------------------
def run_unfilter(raw, F, H, W, bpp, lut=None):
    from dino_tracker_amd import ops
    from dino_tracker_amd._lib import lib
    src = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(DEV)
    sizes = (F * H * W * bpp, 4 * F, ops.png_unfilter_workspace_bytes(F, H, W, bpp))
    assert sizes[2] > 0 and sizes[2] % 256 == 0
    bufs = [guarded(n) for n in sizes]
    out, status, ws = (b[1] for b in bufs)
    status.view(torch.int32).zero_()
    lut_dev = None if lut is None else torch.from_numpy(lut).to(DEV)
    rc = lib().dtk_png_unfilter(src.data_ptr(), F, H, W, bpp, None if lut is None else lut_dev.data_ptr(), out.data_ptr(),
                                status.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib().dtk_last_error()
    torch.cuda.synchronize()
    intact = all(bands_intact(b[0], b[2], n) for b, n in zip(bufs, sizes))
    return out.cpu().numpy().reshape(F, H, W, bpp), status.cpu().numpy().view(np.int32).tolist(), intact


@pytest.mark.parametrize("bpp", [1, 3], ids=["L", "RGB"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_unfilter_three_frames(size, bpp):
    h, w = size
    rng = np.random.default_rng(1000 * h + w + bpp)
    frames = rng.integers(0, 256, size=(3, h, w, bpp), dtype=np.uint8)
    raws = [C.filter_rows(frames[f] if bpp == 3 else frames[f, ..., 0], C.filter_sequence(h, seed=f)) for f in range(3)]
    got, status, intact = run_unfilter(b"".join(raws), 3, h, w, bpp)
    assert intact and status == [0, 0, 0]
    assert np.array_equal(got, frames)
    # random RAW bytes (every predictor value, wrap-arounds): the restatement is the reference; a filter byte 5 in frame 1 only
    if h * w <= 2500:
        pitch = 1 + w * bpp
        raw = rng.integers(0, 256, size=(3, h, pitch), dtype=np.uint8)
        for f in range(3):
            raw[f, :, 0] = C.filter_sequence(h, seed=10 + f)
        raw[1, h // 2, 0] = 5
        want = [R.unfilter(raw[f].tobytes(), h, w, bpp) for f in range(3)]
        got, status, intact = run_unfilter(raw.tobytes(), 3, h, w, bpp)
        assert intact and status == [0, R.PNG_S_FILTER, 0] == [s for _, s in want]
        assert np.array_equal(got, np.stack([px for px, _ in want]))


def test_unfilter_applies_the_palette_table_to_the_output_only():
    h, w = 70, 19
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 256, size=(2, h, w), dtype=np.uint8)
    lut = rng.integers(0, 256, size=(2, 256), dtype=np.uint8)
    raws = [C.filter_rows(idx[f], C.filter_sequence(h, seed=f)) for f in range(2)]
    got, status, intact = run_unfilter(b"".join(raws), 2, h, w, 1, lut)
    assert intact and status == [0, 0]
    assert np.array_equal(got[..., 0], np.stack([lut[f][idx[f]] for f in range(2)]))


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------
def _pillow_png(img, level=6):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG", compress_level=level)
    return buf.getvalue()


def _folder(tmp_path, name, files):
    d = tmp_path / name
    d.mkdir()
    for k, data in enumerate(files):
        (d / f"{k:05d}.png").write_bytes(data)
    return d


@pytest.mark.parametrize("channels", [3, 1], ids=["RGB", "L"])
def test_load_video_equals_the_host_path(tmp_path, monkeypatch, channels):
    from dino_tracker_amd import png_in, video_io
    imgs = [C.picture(70, 45, channels, seed=s) for s in range(3)]
    written = [C.write_png(img, C.filter_sequence(70, seed=k), idat_split=(k * 50,) if k else ()) for k, img in enumerate(imgs)]
    for name, files in (("written", written), ("pillow", [_pillow_png(img, level) for img, level in zip(imgs, (1, 6, 9))])):
        folder = _folder(tmp_path, name, files)
        frames, status = png_in.decode_png(files, DEV, fallback=False, with_status=True)
        assert status.tolist() == [0, 0, 0] and frames.shape == (3, 70, 45, channels)
        assert np.array_equal(frames.cpu().numpy().reshape(np.stack(imgs).shape), np.stack(imgs))
        for resize in (None, (28, 35)):
            monkeypatch.setenv("DTK_PNG_DECODE", "host")
            host = video_io.load_video(folder, resize=resize, device=DEV)
            monkeypatch.setenv("DTK_PNG_DECODE", "device")
            dev = video_io.load_video(folder, resize=resize, device=DEV)
            assert dev.is_cuda and torch.equal(host, dev), (name, resize)


def test_load_video_routes_by_the_switch(tmp_path, monkeypatch):
    """`device` reaches the device decoder, `host` does not; an unknown value is refused"""
    from dino_tracker_amd import png_in, video_io
    folder = _folder(tmp_path, "v", [C.write_png(C.picture(20, 30, 3, seed=s), 4) for s in range(2)])
    calls = []
    real = png_in.decode_planned
    monkeypatch.setattr(png_in, "decode_planned", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setenv("DTK_PNG_DECODE", "host")
    video_io.load_video(folder, device=DEV)
    assert not calls
    monkeypatch.setenv("DTK_PNG_DECODE", "device")
    video_io.load_video(folder, device=DEV)
    assert calls == [1]
    monkeypatch.setenv("DTK_PNG_DECODE", "gpu")
    with pytest.raises(ValueError):
        video_io.load_video(folder, device=DEV)


def _with_wrong_adler(data):
    """the file with the last byte of its zlib stream changed and the chunk's CRC made right again"""
    out = C.SIGNATURE
    for kind, body in R.chunks(data):
        out += C.chunk(kind, body[:-1] + bytes([body[-1] ^ 1]) if kind == b"IDAT" else body)
    return out


def test_a_frame_the_device_rejects_goes_to_pillow_whose_error_surfaces(tmp_path, monkeypatch):
    from dino_tracker_amd import png_in, video_io
    files = [C.write_png(C.picture(20, 30, 3, seed=s), 4) for s in range(3)]
    files[1] = _with_wrong_adler(files[1])
    frames, status = png_in.decode_png(files, DEV, fallback=False, with_status=True)
    assert status.tolist() == [0, R.S_ADLER, 0]
    monkeypatch.setenv("DTK_PNG_DECODE", "device")
    with pytest.raises(OSError):
        video_io.load_video(_folder(tmp_path, "bad", files), device=DEV)
    # a filter byte above 4 is the unfilter kernel's to flag, for its frame only
    files[1] = C.write_png(C.picture(20, 30, 3, seed=9), [0] * 10 + [5] + [0] * 9)
    frames, status = png_in.decode_png(files, DEV, fallback=False, with_status=True)
    assert status.tolist() == [0, R.PNG_S_FILTER, 0]


@pytest.mark.parametrize("kind", ["L", "P"])
def test_load_masks_on_the_device_equals_the_host(tmp_path, monkeypatch, kind):
    from dino_tracker_amd.train import load_masks
    rng = np.random.default_rng(8)
    palette = rng.integers(0, 256, size=768, dtype=np.uint8).tobytes() if kind == "P" else None
    masks = [(rng.integers(0, 256, size=(33, 47), dtype=np.uint8) if kind == "P" else (C.picture(33, 47, 1, seed=s) > 128).astype(np.uint8) * 255)
             for s in range(3)]
    folder = _folder(tmp_path, "m", [C.write_png(m, C.filter_sequence(33, seed=k), palette=palette) for k, m in enumerate(masks)])
    want = load_masks(folder, 20, 30)
    monkeypatch.setenv("DTK_PNG_DECODE", "device")
    got = load_masks(folder, 20, 30, device=DEV)
    assert got.is_cuda and got.dtype == want.dtype and torch.equal(got.cpu(), want)
    full = load_masks(folder, None, None, device=DEV)
    assert torch.equal(full.cpu(), load_masks(folder, None, None))


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_arguments_are_refused_before_anything_is_launched():
    from dino_tracker_amd import ops
    from dino_tracker_amd._lib import lib
    L = lib()
    buf = torch.full((4096,), POISON, dtype=torch.uint8, device=DEV)
    tabd = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    p, t = buf.data_ptr(), tabd.data_ptr()

    def table(*rows):
        return np.ascontiguousarray(np.asarray(rows, dtype=np.int64))

    ok = table([0, 10, 0, 100], [10, 10, 100, 100])
    refused = [
        lambda: L.dtk_inflate(None, 100, t, ok.ctypes.data, 2, 1, p, 1000, p, None),
        lambda: L.dtk_inflate(p, 100, t, None, 2, 1, p, 1000, p, None),
        lambda: L.dtk_inflate(p, 100, t, ok.ctypes.data, 2, 1, None, 1000, p, None),
        lambda: L.dtk_inflate(p, 0, t, ok.ctypes.data, 2, 1, p, 1000, p, None),
        lambda: L.dtk_inflate(p, 100, t, ok.ctypes.data, 0, 1, p, 1000, p, None),
        lambda: L.dtk_inflate(p, 100, t, ok.ctypes.data, 2, 2, p, 1000, p, None),
        lambda: L.dtk_inflate(p, 100, t, ok.ctypes.data, 2, 1, p, 199, p, None),                       # output range past the end
        lambda: L.dtk_inflate(p, 19, t, ok.ctypes.data, 2, 1, p, 1000, p, None),                        # input range past the end
        lambda: L.dtk_adler32(p, 100, t, ok.ctypes.data, 2, p, 199, p, None),
        lambda: L.dtk_adler32(p, 100, t, ok.ctypes.data, 2, None, 1000, p, None),
    ]
    for bad in (table([0, 10, 0, 100], [10, 10, 99, 100]), table([0, 10, 50, 100], [10, 10, 0, 51]), table([-1, 10, 0, 1], [0, 1, 1, 1]),
                table([0, 10, 0, -1], [0, 1, 1, 1])):                                                  # overlaps, negatives
        refused.append(lambda bad=bad: L.dtk_inflate(p, 100, t, bad.ctypes.data, 2, 1, p, 1000, p, None))
    for F, H, W, bpp in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 65536, 1), (1, 65536, 4, 3), (1, 4, 4, 2), (1, 4, 4, 4)):
        assert ops.png_unfilter_workspace_bytes(F, H, W, bpp) == 0
        refused.append(lambda a=(F, H, W, bpp): L.dtk_png_unfilter(p, *a, None, p, p, p, None))
    refused.append(lambda: L.dtk_png_unfilter(None, 1, 4, 4, 1, None, p, p, p, None))
    refused.append(lambda: L.dtk_png_unfilter(p, 1, 4, 4, 1, None, p, p, None, None))
    refused.append(lambda: L.dtk_png_unfilter(p, 1, 4, 4, 3, p, p, p, p, None))                         # a palette table with RGB
    for k, call in enumerate(refused):
        assert call() == E_INVALID, k
        assert L.dtk_last_error()
    torch.cuda.synchronize()
    assert bool((buf == POISON).all())        # nothing was launched
    assert ops.png_unfilter_workspace_bytes(3, 65535, 65535, 3) == (3 * 65535 * 4 + 255) // 256 * 256
