"""GPU: the device PNG encoder (csrc/deflate.hip, dino_tracker_amd/png_out.py) against zlib.decompress, zlib.crc32, zlib.adler32,
Pillow, the original arrays, the plain-Python inflate of tests/png_ref.py and the restated filter stage of tests/png_enc_ref.py -- and,
device -> device, against the decoder (dtk_inflate, dtk_adler32, dtk_png_unfilter, png_in); never against the code under test.
Outputs sit in poisoned buffers between guard bands.

Filter / file sizes (H x W): 1 x 1; 1 x 5 (no row above); 5 x 1 (no left neighbour); 3 x 67 (longer than a wave); 65 x 33; 130 x 7;
32 x 854 (the pipeline's row length, ten bytes a thread).  DEFLATE lengths sit around the match limits (258) and the segment size S."""
import io
import random
import struct
import zlib

import numpy as np
import pytest
import torch

import png_enc_ref as E
import png_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xA5
GUARD = 4096
SIZES = [(1, 1), (1, 5), (5, 1), (3, 67), (65, 33), (130, 7), (32, 854)]
E_INVALID = -1
S = 32768


def L():
    from dino_tracker_amd._lib import lib
    return lib()


def guarded(nbytes):
    """(whole buffer filled with POISON, the 256-byte aligned view of `nbytes` between two guard bands, its start)"""
    whole = torch.full((GUARD + nbytes + 256 + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(whole.data_ptr() + GUARD)) % 256
    return whole, whole[start:start + nbytes], start


def bands_intact(whole, start, nbytes):
    return bool((whole[:start] == POISON).all()) and bool((whole[start + nbytes:] == POISON).all())


def stream_handle():
    return torch.cuda.current_stream().cuda_stream


def upload(data):
    return torch.from_numpy(np.frombuffer(bytes(data) or b"\x00", dtype=np.uint8).copy()).to(DEV)


def test_segment_size_is_the_headers():
    from dino_tracker_amd import ops
    assert ops.DEFLATE_SEGMENT == S


# ---- 1. the filter stage -----------------------------------------------------------------------------------------------------------
def frames_for(h, w, bpp, seed):
    """three different frames: noise (wrap-arounds, every predictor value), a smooth picture (every filter wins rows), flat bands
    (rows whose costs tie)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    smooth = np.stack([(3 * x + 5 * y * (c + 1) + rng.integers(0, 6, size=(h, w))) % 256 for c in range(bpp)], axis=-1)
    flat = np.zeros((h, w, bpp), dtype=np.int64)
    flat[h // 3:] = 7
    flat[2 * h // 3:, w // 2:] = 250
    return np.stack([rng.integers(0, 256, size=(h, w, bpp)), smooth, flat]).astype(np.uint8)


def run_filter(frames, kind):
    F, H, W, bpp = frames.shape
    src = torch.from_numpy(frames).to(DEV)
    n = F * H * (1 + W * bpp)
    whole, raw, start = guarded(n)
    rc = L().dtk_png_filter(src.data_ptr(), F, H, W, bpp, kind, raw.data_ptr(), stream_handle())
    assert rc == 0, L().dtk_last_error()
    torch.cuda.synchronize()
    return raw, bands_intact(whole, start, n)


@pytest.mark.parametrize("bpp", [1, 3], ids=["L", "RGB"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_three_frames(size, bpp):
    from dino_tracker_amd import ops
    h, w = size
    frames = frames_for(h, w, bpp, seed=1000 * h + w + bpp)
    picked = set()
    for kind in (0, 1, 2, 3, 4, 5):
        raw, intact = run_filter(frames, kind)
        want = b"".join(E.filter_image_fast(frames[f], kind) for f in range(3))
        got = raw.cpu().numpy().tobytes()
        assert intact and got == want, (size, bpp, kind)
        if h * w <= 600:      # the plain-Python loops on the small sizes, the numpy form of the same rule on all
            assert want == b"".join(E.filter_image(frames[f], kind) for f in range(3))
        status = torch.zeros(3, dtype=torch.int32, device=DEV)
        back = ops.png_unfilter(raw, 3, h, w, bpp, status)
        assert status.tolist() == [0, 0, 0] and np.array_equal(back.cpu().numpy(), frames), (size, bpp, kind)
        if kind == 5:
            picked = set(got[:: 1 + w * bpp])
    assert picked <= {0, 1, 2, 3, 4}
    if h >= 32:
        assert len(picked) >= 3      # the adaptive rule really chooses


# ---- 2. DEFLATE ----------------------------------------------------------------------------------------------------------------------
def fibonacci_bytes():
    """17 710 bytes: 20 values with counts 1, 1, 2, 3, ... 6765, shuffled: a Huffman code without a length limit is deeper than 15"""
    counts, a, b = [], 1, 1
    for _ in range(20):
        counts.append(a)
        a, b = b, a + b
    data = np.concatenate([np.full(c, 40 + 3 * k, dtype=np.uint8) for k, c in enumerate(counts)])
    assert data.size == 17710
    np.random.default_rng(20).shuffle(data)
    return data.tobytes()


def make_inputs():
    rng = np.random.default_rng(77)
    inputs = [(f"run_{n}", bytes([0x5A]) * n) for n in (0, 1, 2, 3, 258, 259, 260)]
    for n in (S - 1, S, S + 1, 2 * S + 17):
        inputs.append((f"zeros_{n}", bytes(n)))
        inputs.append((f"period3_{n}", (b"\x11\x7f\xe0" * (n // 3 + 1))[:n]))
        inputs.append((f"random_{n}", rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()))
        inputs.append((f"geometric_{n}", np.minimum(255, rng.geometric(0.25, size=n) - 1).astype(np.uint8).tobytes()))
    inputs.append(("fibonacci_17710", fibonacci_bytes()))
    return inputs


INPUTS = make_inputs()
NAMES = [name for name, _ in INPUTS]


def run_deflate(datas, wrapper, seed=None, gap=0, capacity=None):
    """The inputs lie in the input buffer in a shuffled order (seed) with `gap` bytes of noise between them.  -> (the streams as byte
    strings, or None when the output did not fit; offsets; needed; intact: the guard bands of output, offsets and needed; the whole
    output range as bytes)"""
    order = list(range(len(datas)))
    if seed is not None:
        random.Random(seed).shuffle(order)
    table = np.zeros((len(datas), 2), dtype=np.int64)
    blob, at = bytearray(), 1                       # an odd first offset
    blob += b"\xEE"
    for k in order:
        table[k] = (at, len(datas[k]))
        blob += datas[k] + bytes([0xEE]) * gap
        at += len(datas[k]) + gap
    src, tab = upload(blob), torch.from_numpy(table).to(DEV)
    cap = sum(int(L().dtk_deflate_bound(len(d))) for d in datas) if capacity is None else capacity
    ws_bytes = int(L().dtk_deflate_workspace_bytes(table.ctypes.data, len(datas)))
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    bufs = [guarded(n) for n in (max(cap, 1), 8 * (len(datas) + 1), 8, ws_bytes)]
    out, offsets, needed, ws = (b[1] for b in bufs)
    rc = L().dtk_deflate(src.data_ptr(), src.numel(), tab.data_ptr(), table.ctypes.data, len(datas), wrapper, out.data_ptr(), cap,
                         offsets.data_ptr(), needed.data_ptr(), ws.data_ptr(), stream_handle())
    assert rc == 0, L().dtk_last_error()
    torch.cuda.synchronize()
    intact = all(bands_intact(b[0], b[2], n) for b, n in zip(bufs, (max(cap, 1), 8 * (len(datas) + 1), 8, ws_bytes)))
    offs = offsets.cpu().numpy().view(np.int64).tolist()
    need = int(needed.cpu().numpy().view(np.int64)[0])
    host = out.cpu().numpy().tobytes()
    streams = [host[a:b] for a, b in zip(offs[:-1], offs[1:])] if need <= cap else None
    return streams, offs, need, intact, host


def device_round_trip(streams, datas, wrapper):
    """dtk_inflate (+ dtk_adler32) of the streams: -> ([output bytes], [status])"""
    table = np.zeros((len(streams), 4), dtype=np.int64)
    table[:, 0] = np.concatenate(([0], np.cumsum([len(s) for s in streams])))[:-1]
    table[:, 1] = [len(s) for s in streams]
    table[:, 2] = np.concatenate(([0], np.cumsum([len(d) for d in datas])))[:-1]
    table[:, 3] = [len(d) for d in datas]
    total = max(1, sum(len(d) for d in datas))
    src, tab = upload(b"".join(streams)), torch.from_numpy(table).to(DEV)
    out = torch.full((total,), POISON, dtype=torch.uint8, device=DEV)
    status = torch.full((len(streams),), -1, dtype=torch.int32, device=DEV)
    rc = L().dtk_inflate(src.data_ptr(), src.numel(), tab.data_ptr(), table.ctypes.data, len(streams), wrapper, out.data_ptr(), total,
                         status.data_ptr(), stream_handle())
    assert rc == 0, L().dtk_last_error()
    if wrapper:
        rc = L().dtk_adler32(src.data_ptr(), src.numel(), tab.data_ptr(), table.ctypes.data, len(streams), out.data_ptr(), total,
                             status.data_ptr(), stream_handle())
        assert rc == 0, L().dtk_last_error()
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    return [host[int(r[2]):int(r[2] + r[3])] for r in table], status.tolist()


def check_stream(name, data, stream, wrapper):
    n = len(data)
    assert zlib.decompress(stream, 15 if wrapper else -15) == data, name
    if wrapper:
        assert stream[:2] == b"\x78\x01" and struct.unpack(">I", stream[-4:])[0] == zlib.adler32(data), name
    bound = int(L().dtk_deflate_bound(n))
    assert bound <= n + n // 1024 + 64
    print(f"{name}: {n} -> {len(stream)} bytes ({len(stream) / max(n, 1):.4f} n), bound {bound}, wrapper {wrapper}")
    assert len(stream) <= bound - (0 if wrapper else 6), name                          # the stored fall-back
    if name.startswith(("zeros_", "period3_")) and n >= S:
        assert len(stream) <= 0.02 * n, name                                           # matches of length 258
    if name.startswith("geometric_"):
        assert len(stream) <= 0.60 * n, name                                           # dynamic codes
    if n <= S + 1:
        body, status, stats = R.inflate(stream, n, wrapper=bool(wrapper))
        assert status == 0 and body == data, (name, status)
        assert stats["largest_distance"] <= S and stats["longest_code"] <= 15
        if name.startswith(("zeros_", "period3_")) and n >= 1000:
            assert stats["tokens"] < n // 100, (name, stats)


@pytest.mark.parametrize("name", NAMES)
def test_deflate_each_input_alone(name):
    data = dict(INPUTS)[name]
    for wrapper in (1, 0):
        streams, offs, need, intact, host = run_deflate([data], wrapper)
        assert intact and offs[0] == 0 and offs[-1] == need == len(streams[0])
        check_stream(name, data, streams[0], wrapper)
        outs, status = device_round_trip(streams, [data], wrapper)
        assert status == [0] and outs[0] == data, (name, status)
        again, offs2, need2, intact2, _ = run_deflate([data], wrapper)
        assert intact2 and again == streams and offs2 == offs and need2 == need          # a pure function of the input


def test_deflate_all_inputs_in_one_call_shuffled():
    datas = [d for _, d in INPUTS]
    alone = {}
    for wrapper in (1, 0):
        streams, offs, need, intact, host = run_deflate(datas, wrapper, seed=9, gap=5)
        assert intact and offs[0] == 0 and offs[-1] == need == sum(len(s) for s in streams)
        assert all(b - a == len(s) for a, b, s in zip(offs[:-1], offs[1:], streams))
        assert bytes(host[need:]) == bytes([POISON]) * (len(host) - need)              # nothing behind the last stream
        for (name, data), stream in zip(INPUTS, streams):
            assert zlib.decompress(stream, 15 if wrapper else -15) == data, name
        outs, status = device_round_trip(streams, datas, wrapper)
        assert status == [0] * len(datas) and outs == datas
        again = run_deflate(datas, wrapper, seed=10, gap=2)[0]                          # where an input lies does not change its stream
        assert again == streams
        alone[wrapper] = streams
    assert all(z[2:-4] == r for z, r in zip(alone[1], alone[0]))                        # the wrapper wraps the same bytes


def test_deflate_capacity_protocol():
    datas = [dict(INPUTS)[k] for k in ("geometric_%d" % (S + 1), "run_3", "zeros_%d" % S, "random_%d" % (S - 1))]
    streams, offs, need, intact, _ = run_deflate(datas, 1, seed=3)
    assert intact and streams is not None
    short, offs2, need2, intact2, host = run_deflate(datas, 1, seed=3, capacity=need - 1)
    assert short is None and intact2 and need2 == need and offs2 == offs               # needed is exact, the offsets are written
    assert host == bytes([POISON]) * (need - 1)                                         # and nothing else
    exact, offs3, need3, intact3, _ = run_deflate(datas, 1, seed=3, capacity=need)
    assert intact3 and exact == streams and need3 == need


def test_png_out_deflate_wrapper():
    from dino_tracker_amd import png_out
    datas = [dict(INPUTS)[k] for k in ("run_0", "fibonacci_17710", "period3_%d" % (S + 1))]
    for wrapper in (True, False):
        got = png_out.deflate(datas, DEV, wrapper)
        assert [zlib.decompress(s, 15 if wrapper else -15) for s in got] == datas


# ---- 3. CRC-32 -----------------------------------------------------------------------------------------------------------------------
def test_crc32_ranges_at_odd_offsets():
    lengths = [0, 1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, (1 << 20) + 3]
    rng = np.random.default_rng(5)
    blob = rng.integers(0, 256, size=sum(lengths) + 2 * len(lengths) + 1, dtype=np.uint8).tobytes()
    table, at = np.zeros((len(lengths), 2), dtype=np.int64), 1
    for k, n in enumerate(lengths):
        table[k] = (at, n)
        at += n + (1 if (at + n) % 2 == 0 else 2)          # every range starts at an odd offset
    assert all(int(o) % 2 == 1 for o in table[:, 0])
    src, tab = upload(blob), torch.from_numpy(table).to(DEV)
    whole, out, start = guarded(4 * len(lengths))
    rc = L().dtk_crc32(src.data_ptr(), src.numel(), tab.data_ptr(), table.ctypes.data, len(lengths), out.data_ptr(), stream_handle())
    assert rc == 0, L().dtk_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32).tolist()
    want = [zlib.crc32(blob[int(o):int(o + n)]) for o, n in table]
    assert bands_intact(whole, start, 4 * len(lengths)) and got == want
    from dino_tracker_amd import ops
    assert ops.crc32(src, table[::-1].copy()).tolist() == want[::-1]


# ---- 4. whole files ------------------------------------------------------------------------------------------------------------------
def picture_frames(h, w, bpp):
    """three different frames of a rendered look: gradients, flat regions, a noisy band"""
    rng = np.random.default_rng(h * 7 + w + bpp)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for f in range(3):
        img = np.stack([((x * (c + 2 + f)) // 3 + (y * (f + 1)) // 2) % 256 for c in range(bpp)], axis=-1)
        img[(y // 8 + x // 16 + f) % 3 == 0] = 30 + 60 * f
        img[h // 2: h // 2 + max(1, h // 8)] = rng.integers(0, 256, size=img[h // 2: h // 2 + max(1, h // 8)].shape)
        out.append(img)
    return np.stack(out).astype(np.uint8)


FILE_CASES = [(h, w, bpp) for h, w in SIZES for bpp in (1, 3)] + [(64, 1023, 1), (480, 854, 3)]


@pytest.mark.parametrize("case", FILE_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_whole_files(case):
    from PIL import Image
    from dino_tracker_amd import ops, png_in, png_out
    h, w, bpp = case
    if case == (64, 1023, 1):
        assert h * (1 + w * bpp) == 2 * S
    frames = picture_frames(h, w, bpp)
    dev_frames = torch.from_numpy(frames).to(DEV)
    # the library call, in a poisoned buffer
    header = upload(png_out.png_header(h, w, bpp))
    cap = ops.png_worst_case_bytes(3, h, w, bpp)
    ws_bytes = ops.png_encode_workspace_bytes(3, h, w, bpp)
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    sizes = (cap, 8 * 4, 8, ws_bytes)
    bufs = [guarded(n) for n in sizes]
    out, offsets, needed, ws = (b[1] for b in bufs)
    rc = L().dtk_png_encode(dev_frames.data_ptr(), 3, h, w, bpp, 5, header.data_ptr(), out.data_ptr(), cap, offsets.data_ptr(),
                            needed.data_ptr(), ws.data_ptr(), stream_handle())
    assert rc == 0, L().dtk_last_error()
    torch.cuda.synchronize()
    assert all(bands_intact(b[0], b[2], n) for b, n in zip(bufs, sizes))
    offs = offsets.cpu().numpy().view(np.int64).tolist()
    need = int(needed.cpu().numpy().view(np.int64)[0])
    host = out.cpu().numpy().tobytes()
    assert offs[0] == 0 and offs[-1] == need <= cap and host[need:] == bytes([POISON]) * (cap - need)
    files = [host[a:b] for a, b in zip(offs[:-1], offs[1:])]
    assert files == list(png_out.png_files(dev_frames if bpp == 3 else dev_frames[..., 0]))       # the Python path gives the same bytes
    mode = "L" if bpp == 1 else "RGB"
    raw_bytes = h * (1 + w * bpp)
    for f, data in enumerate(files):
        chunks = E.walk(data)
        assert [k for k, *_ in chunks] == [b"IHDR", b"IDAT", b"IEND"], case
        assert all(stored == computed for _, _, stored, computed in chunks), case
        assert data[:33] == png_out.png_header(h, w, bpp)
        z = chunks[1][1]
        assert zlib.decompress(z) == E.filter_image_fast(frames[f], 5)                 # the filter stage, through zlib
        assert len(z) <= int(L().dtk_deflate_bound(raw_bytes))
        Image.open(io.BytesIO(data)).verify()
        img = Image.open(io.BytesIO(data))
        assert img.mode == mode and np.array_equal(np.asarray(img).reshape(h, w, bpp), frames[f]), (case, f)
        head, why = png_in.parse_png(data)
        assert why is None and (head.height, head.width, head.mode) == (h, w, mode)
    back, status = png_in.decode_png(files, DEV, fallback=False, with_status=True)
    assert status.tolist() == [0, 0, 0] and np.array_equal(back.cpu().numpy(), frames)
    print(f"{case}: files of {[len(d) for d in files]} bytes for {h * w * bpp} pixel bytes each")


def test_forced_filters_and_capacity_through_ops():
    from PIL import Image
    from dino_tracker_amd import ops, png_out
    frames = picture_frames(40, 50, 3)
    dev_frames = torch.from_numpy(frames).to(DEV)
    header = upload(png_out.png_header(40, 50, 3))
    sizes = {}
    for name, code in png_out.FILTERS.items():
        data, offs = png_out.encode_png(dev_frames, name)
        offs = offs.tolist()
        host = data.cpu().numpy().tobytes()
        for f in range(3):
            blob = host[offs[f]:offs[f + 1]]
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(blob))), frames[f])
            raw = zlib.decompress(E.walk(blob)[1][1])
            assert raw == E.filter_image_fast(frames[f], code), name
        sizes[name] = offs[-1]
    # a first buffer that is too small: one retry with the exact size, the same bytes
    want, want_offs = ops.png_encode(dev_frames, header)
    got, got_offs = ops.png_encode(dev_frames, header, capacity=100)
    assert torch.equal(want, got) and torch.equal(want_offs, got_offs)


# ---- 5. entry points -----------------------------------------------------------------------------------------------------------------
def test_save_video_png_container(tmp_path):
    from PIL import Image
    from dino_tracker_amd import video_io, visualize
    frames = picture_frames(36, 52, 3)
    written = visualize.save_video(torch.from_numpy(frames).to(DEV), str(tmp_path / "clip.mp4"), container="png")
    assert written == str(tmp_path / "clip")
    assert sorted(p.name for p in (tmp_path / "clip").iterdir()) == ["00000.png", "00001.png", "00002.png"]
    host = tmp_path / "host"
    host.mkdir()
    for k, img in enumerate(frames):
        Image.fromarray(img).save(host / f"{k:05d}.png")
    got, want = video_io.load_video(written, device=DEV), video_io.load_video(host, device=DEV)
    assert torch.equal(got, want)
    assert torch.equal((got * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu(), torch.from_numpy(frames))
    again = visualize.save_video(frames, str(tmp_path / "fromnumpy.mp4"), container="png")       # a numpy array is uploaded
    assert (tmp_path / "fromnumpy" / "00002.png").read_bytes() == (tmp_path / "clip" / "00002.png").read_bytes() and again
    with pytest.raises(ValueError):
        visualize.save_video(frames, str(tmp_path / "x.mp4"), container="gif")


def test_save_masks_routes_by_the_switch(tmp_path, monkeypatch):
    from dino_tracker_amd import fg_mask, png_out
    from dino_tracker_amd.train import load_masks
    rng = np.random.default_rng(12)
    y, x = np.mgrid[0:33, 0:47]
    mask = torch.from_numpy(np.stack([(((x - 20 - s) ** 2 + (y - 15) ** 2 < 120) * 255).astype(np.uint8) for s in range(3)]))
    mask[2, :4] = torch.from_numpy(rng.integers(0, 256, size=(4, 47), dtype=np.uint8))
    calls = []
    real = png_out.write_png_frames
    monkeypatch.setattr(png_out, "write_png_frames", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.delenv("DTK_PNG_ENCODE", raising=False)
    fg_mask.save_masks(mask.to(DEV), str(tmp_path / "default"))
    monkeypatch.setenv("DTK_PNG_ENCODE", "host")
    fg_mask.save_masks(mask.to(DEV), str(tmp_path / "host"))
    assert not calls                                                                     # neither reaches the library
    monkeypatch.setenv("DTK_PNG_ENCODE", "device")
    fg_mask.save_masks(mask.to(DEV), str(tmp_path / "device"))
    fg_mask.save_masks(mask, str(tmp_path / "device_from_host"))                         # a host tensor is uploaded
    assert calls == [1, 1]
    want = load_masks(tmp_path / "host", None, None)
    assert torch.equal(want, mask)
    for name in ("default", "device", "device_from_host"):
        assert torch.equal(load_masks(tmp_path / name, None, None), want), name
        assert torch.equal(load_masks(tmp_path / name, 20, 30), load_masks(tmp_path / "host", 20, 30)), name
    monkeypatch.setenv("DTK_PNG_ENCODE", "gpu")
    with pytest.raises(ValueError):
        fg_mask.save_masks(mask.to(DEV), str(tmp_path / "bad"))


def test_arguments_are_refused_before_anything_is_launched():
    from dino_tracker_amd import ops
    lib = L()
    buf = torch.full((8192,), POISON, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()

    def table(*rows):
        return np.ascontiguousarray(np.asarray(rows, dtype=np.int64))

    ok = table([0, 100], [100, 50])
    refused = [
        lambda: lib.dtk_deflate(None, 1000, p, ok.ctypes.data, 2, 1, p, 4096, p, p, p, None),
        lambda: lib.dtk_deflate(p, 1000, None, ok.ctypes.data, 2, 1, p, 4096, p, p, p, None),
        lambda: lib.dtk_deflate(p, 1000, p, None, 2, 1, p, 4096, p, p, p, None),
        lambda: lib.dtk_deflate(p, 1000, p, ok.ctypes.data, 2, 1, None, 4096, p, p, p, None),
        lambda: lib.dtk_deflate(p, 1000, p, ok.ctypes.data, 2, 1, p, 4096, None, p, p, None),
        lambda: lib.dtk_deflate(p, 1000, p, ok.ctypes.data, 2, 1, p, 4096, p, None, p, None),
        lambda: lib.dtk_deflate(p, 1000, p, ok.ctypes.data, 2, 1, p, 4096, p, p, None, None),
        lambda: lib.dtk_deflate(p, 0, p, ok.ctypes.data, 2, 1, p, 4096, p, p, p, None),
        lambda: lib.dtk_deflate(p, 1000, p, ok.ctypes.data, 0, 1, p, 4096, p, p, p, None),
        lambda: lib.dtk_deflate(p, 1000, p, ok.ctypes.data, 2, 2, p, 4096, p, p, p, None),
        lambda: lib.dtk_deflate(p, 149, p, ok.ctypes.data, 2, 1, p, 4096, p, p, p, None),                 # a range past the end
        lambda: lib.dtk_crc32(None, 1000, p, ok.ctypes.data, 2, p, None),
        lambda: lib.dtk_crc32(p, 1000, p, None, 2, p, None),
        lambda: lib.dtk_crc32(p, 1000, p, ok.ctypes.data, 2, None, None),
        lambda: lib.dtk_crc32(p, 149, p, ok.ctypes.data, 2, p, None),
        lambda: lib.dtk_crc32(p, 1000, p, ok.ctypes.data, 0, p, None),
    ]
    for bad in (table([-1, 10], [0, 1]), table([0, -1], [0, 1]), table([0, (1 << 30) + 1], [0, 1])):
        refused.append(lambda bad=bad: lib.dtk_deflate(p, 1 << 40, p, bad.ctypes.data, 2, 1, p, 4096, p, p, p, None))
        assert lib.dtk_deflate_workspace_bytes(bad.ctypes.data, 2) == 0 or bad[0, 0] == -1
    assert lib.dtk_deflate_workspace_bytes(None, 2) == 0 and lib.dtk_deflate_workspace_bytes(ok.ctypes.data, 0) == 0
    for F, H, W, bpp in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 3), (1, 4, 65536, 1), (1, 65536, 4, 3), (1, 4, 4, 2), (1, 4, 4, 4),
                         (1, 65535, 65535, 3)):
        assert ops.png_encode_workspace_bytes(F, H, W, bpp) == 0
        refused.append(lambda a=(F, H, W, bpp): lib.dtk_png_filter(p, *a, 5, p, None))
        refused.append(lambda a=(F, H, W, bpp): lib.dtk_png_encode(p, *a, 5, p, p, 4096, p, p, p, None))
    for flt in (-1, 6):
        refused.append(lambda flt=flt: lib.dtk_png_filter(p, 1, 4, 4, 1, flt, p, None))
        refused.append(lambda flt=flt: lib.dtk_png_encode(p, 1, 4, 4, 1, flt, p, p, 4096, p, p, p, None))
    refused.append(lambda: lib.dtk_png_filter(None, 1, 4, 4, 1, 5, p, None))
    refused.append(lambda: lib.dtk_png_filter(p, 1, 4, 4, 1, 5, None, None))
    for hole in range(6):
        args = [p, p, p, p, p, p]
        args[hole] = None
        refused.append(lambda a=args: lib.dtk_png_encode(a[0], 1, 4, 4, 1, 5, a[1], a[2], 4096, a[3], a[4], a[5], None))
    for k, call in enumerate(refused):
        assert call() == E_INVALID, k
        assert lib.dtk_last_error()
    torch.cuda.synchronize()
    assert bool((buf == POISON).all())        # nothing was launched
    assert lib.dtk_deflate_bound(0) == 11 and lib.dtk_deflate_bound(S) == S + 11 and lib.dtk_deflate_bound(S + 1) == S + 1 + 16
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.png_filter(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
