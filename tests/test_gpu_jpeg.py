"""GPU: the device JPEG encoder (csrc/jpeg.hip, dino_tracker_amd/video_out.py) against the numpy restatement of docs/JPEG.md in
tests/jpeg_ref.py -- never against the code under test, and without Pillow's ENCODER: the restatement's own agreement with Pillow is
the CPU file's business (tests/test_jpeg_reference.py).  Everything is an equality: the arithmetic is integer.

Sizes (H x W) are the CPU file's, chosen where the encoder can go wrong -- one pixel, an odd height (a row repeated to make the
count even), heights that are even but no multiple of 16 (the downsampled chroma row repeats, not the plane), widths that are no
multiple of 8 or 16 (dummy blocks), more MCUs than one transform workgroup or one restart interval holds, a last interval that is
not full -- plus 16 x 1920: one MCU row at 1080p width."""
import io
import os
import pickle

import numpy as np
import pytest
import torch

import jpeg_ref as J

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (2, 16), (8, 16), (17, 9), (16, 16), (33, 50), (48, 160), (130, 23), (200, 40), (32, 854)]
POISON = 0xA5
GUARD = 4096   # bytes


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # a copy: the references are read-only


_REF = {}


def ref(kind, h, w, q, seed=0):
    """(picture, coefficients, file) of the restatement, computed once per case and never modified"""
    key = (kind, h, w, q, seed)
    if key not in _REF:
        img = J.picture(kind, h, w, seed)
        coef = J.coefficients(img, q)
        data = J.header(h, w, q) + J.scan(coef) + b"\xff\xd9"
        for a in (img, coef):
            a.setflags(write=False)
        _REF[key] = (img, coef, data)
    return _REF[key]


def qtables(q):
    from dino_tracker_amd import video_out
    return dev(video_out.quant_tables(q))


# ---- 1. coefficients -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES + [(16, 1920)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_coefficients_equal_the_restatement(size):
    from dino_tracker_amd import ops
    h, w = size
    for kind, q in (("noise", 90), ("ramp", 100), ("checker", 5), ("pm1", 10)):
        img, want, _ = ref(kind, h, w, q)
        got = ops.jpeg_coefficients(dev(img)[None], qtables(q))
        assert tuple(got.shape) == (1,) + want.shape
        assert torch.equal(got[0].cpu(), torch.from_numpy(want.copy())), (kind, q, size)


def test_coefficients_of_several_frames():
    from dino_tracker_amd import ops
    imgs = np.stack([J.picture("noise", 33, 50, seed=s) for s in range(3)])
    got = ops.jpeg_coefficients(dev(imgs), qtables(75)).cpu().numpy()
    for f in range(3):
        np.testing.assert_array_equal(got[f], J.coefficients(imgs[f], 75))


# ---- 2. streams, with guard bands around everything the call writes ------------------------------------------------------------
def guarded(nbytes, dtype=torch.uint8):
    """(whole buffer filled with POISON, the 256-byte aligned view of `nbytes` between two guard bands)"""
    whole = torch.full((GUARD + nbytes + 256 + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(whole.data_ptr() + GUARD)) % 256
    return whole, whole[start:start + nbytes], start


def bands_intact(whole, start, nbytes):
    return bool((whole[:start] == POISON).all()) and bool((whole[start + nbytes:] == POISON).all())


def raw_encode(imgs, q, capacity):
    """dtk_jpeg_encode through ctypes on guarded buffers -> (rc, out bytes as written, offsets, needed, all bands intact)"""
    from dino_tracker_amd import ops, video_out
    from dino_tracker_amd._lib import lib
    F, H, W = imgs.shape[:3]
    frames, qt = dev(imgs), qtables(q)
    head = video_out.jpeg_header(H, W, q)
    header = dev(np.frombuffer(head, dtype=np.uint8))
    ws_bytes = ops.jpeg_workspace_bytes(F, H, W)
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    bufs = [guarded(capacity), guarded(8 * (F + 1)), guarded(8), guarded(ws_bytes)]
    (out, offsets, needed, ws) = (b[1] for b in bufs)
    rc = lib().dtk_jpeg_encode(frames.data_ptr(), F, H, W, qt.data_ptr(), header.data_ptr(), len(head), out.data_ptr(), capacity,
                               offsets.data_ptr(), needed.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    intact = all(bands_intact(b[0], b[2], n) for b, n in zip(bufs, (capacity, 8 * (F + 1), 8, ws_bytes)))
    return (rc, out.cpu().numpy().tobytes(), offsets.cpu().numpy().view(np.int64).tolist(),
            int(needed.cpu().numpy().view(np.int64)[0]), intact)


@pytest.mark.parametrize("q", [5, 90, 100])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_frame_streams_equal_the_restatement(size, q):
    from PIL import Image
    h, w = size
    for kind in ("noise", "checker") if q != 5 else ("noise", "pm1"):
        img, _, want = ref(kind, h, w, q)
        rc, out, offsets, needed, intact = raw_encode(img[None], q, len(want) + 64)
        assert rc == 0 and intact
        assert offsets == [0, len(want)] and needed == len(want)
        assert out[:len(want)] == want, (kind, size, q)
        assert out[len(want):] == bytes([POISON]) * 64
        Image.open(io.BytesIO(out[:needed])).load()   # decodes


@pytest.mark.parametrize("q", [5, 90, 100])
@pytest.mark.parametrize("size", [(17, 9), (33, 50), (200, 40), (32, 854)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_frames_in_one_call(size, q):
    """three different contents; at 33 x 50 (12 MCUs), 200 x 40 (39) and 32 x 854 (108) the last interval is not full"""
    from PIL import Image
    h, w = size
    refs = [ref(kind, h, w, q, seed) for kind, seed in (("noise", 1), ("ramp", 0), ("checker", 0))]
    want = b"".join(r[2] for r in refs)
    ends = np.cumsum([0] + [len(r[2]) for r in refs]).tolist()
    rc, out, offsets, needed, intact = raw_encode(np.stack([r[0] for r in refs]), q, len(want))
    assert rc == 0 and intact and offsets == ends and needed == len(want)
    assert out == want
    for a, b in zip(ends[:-1], ends[1:]):
        assert Image.open(io.BytesIO(out[a:b])).size == (w, h)
        Image.open(io.BytesIO(out[a:b])).load()


def test_pillow_encoder_on_this_machine(capsys):
    """printed, not asserted: whether this machine's Pillow gives the device's bytes (its libjpeg build is not ours to pin)"""
    from PIL import Image, features
    from dino_tracker_amd import video_out
    same, total, why = 0, 0, ""
    for h, w in SIZES:
        img = J.picture("noise", h, w)
        data, offsets = video_out.encode_jpeg(dev(img)[None], 90)
        assert offsets.tolist() == [0, data.numel()]
        try:
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "JPEG", quality=90, subsampling=2, restart_marker_blocks=J.RESTART)
            same += buf.getvalue() == data.cpu().numpy().tobytes()
            total += 1
        except Exception as e:   # no JPEG codec, or no restart_marker_blocks
            why = repr(e)
    with capsys.disabled():
        print(f"\n[jpeg] Pillow {Image.__version__}, libjpeg {features.version('jpg')}: {same} of {total} files byte-equal to the "
              f"device's {why}")


# ---- 3. capacity ---------------------------------------------------------------------------------------------------------------
def test_short_capacity_reports_the_size_and_writes_nothing():
    from dino_tracker_amd import ops, video_out
    imgs = np.stack([ref("noise", 33, 50, 90, s)[0] for s in (1, 2)])
    want = b"".join(ref("noise", 33, 50, 90, s)[2] for s in (1, 2))
    for capacity in (len(want) - 1, 16):
        rc, out, offsets, needed, intact = raw_encode(imgs, 90, capacity)
        assert rc == 0 and intact and needed == len(want) and offsets[-1] == len(want)
        assert out == bytes([POISON]) * capacity            # nothing at all was written
    head = dev(np.frombuffer(video_out.jpeg_header(33, 50, 90), dtype=np.uint8))
    for capacity in (16, len(want) - 1, len(want), None):    # the wrapper retries once with the reported size
        data, offsets = ops.jpeg_encode(dev(imgs), qtables(90), head, capacity)
        assert data.cpu().numpy().tobytes() == want and offsets.tolist() == [0, len(ref("noise", 33, 50, 90, 1)[2]), len(want)]


def test_batches_and_the_guessed_capacity(monkeypatch):
    """encode_jpeg in batches of one frame, with a first capacity far too small: the same stream"""
    from dino_tracker_amd import video_out
    imgs = np.stack([ref("noise", 48, 160, 100, s)[0] for s in (0, 1, 2)])
    want = [ref("noise", 48, 160, 100, s)[2] for s in (0, 1, 2)]
    monkeypatch.setattr(video_out, "WORKSPACE_BUDGET", 1)
    monkeypatch.setattr(video_out, "WORST_CASE_LIMIT", 0)
    monkeypatch.setattr(video_out, "GUESS_BYTES_PER_PIXEL", 0.01)
    data, offsets = video_out.encode_jpeg(dev(imgs), 100)
    assert data.cpu().numpy().tobytes() == b"".join(want)
    assert offsets.tolist() == np.cumsum([0] + [len(x) for x in want]).tolist()
    assert list(video_out.jpeg_files(imgs, 100)) == want     # numpy frames are uploaded


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    from dino_tracker_amd import ops, video_out
    from dino_tracker_amd._lib import lib
    h = lib()
    whole, buf, start = guarded(1 << 16)
    p = buf.data_ptr()
    for F, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 65536, 8), (1, 8, 65536), (-1, 8, 8)):
        assert h.dtk_jpeg_workspace_bytes(F, H, W) == 0
        assert h.dtk_jpeg_coefficients(p, F, H, W, p, p, None) == -1 and b"jpeg_coefficients" in h.dtk_last_error()
        assert h.dtk_jpeg_encode(p, F, H, W, p, p, 8, p, 1 << 16, p, p, p, None) == -1 and b"jpeg_encode" in h.dtk_last_error()
    for hole in range(3):
        args = [p, 1, 8, 8, p, p, None]
        args[(0, 4, 5)[hole]] = None
        assert h.dtk_jpeg_coefficients(*args) == -1 and b"null pointer" in h.dtk_last_error()
    for hole in (0, 4, 5, 7, 9, 10, 11):
        args = [p, 1, 8, 8, p, p, 8, p, 1 << 16, p, p, p, None]
        args[hole] = None
        assert h.dtk_jpeg_encode(*args) == -1 and b"null pointer" in h.dtk_last_error()
    assert h.dtk_jpeg_encode(p, 1, 8, 8, p, p, 0, p, 1 << 16, p, p, p, None) == -1
    torch.cuda.synchronize()
    assert bool((whole == POISON).all())
    assert h.dtk_jpeg_workspace_bytes(1, 65535, 65535) > 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.jpeg_coefficients(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), qtables(90))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.jpeg_encode(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), qtables(90), qtables(90).reshape(-1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video_out.encode_jpeg(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(TypeError):
        video_out.encode_jpeg(torch.zeros(1, 8, 8, 3, device=DEV))
    with pytest.raises(ValueError, match="container"):
        from dino_tracker_amd import visualize
        visualize.save_video(torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV), "x.mp4", container="mkv")


# ---- 5. end to end: the command lines ------------------------------------------------------------------------------------------
def capture(monkeypatch, module, name, store):
    original = getattr(module, name)

    def wrapped(*args, **kwargs):
        out = original(*args, **kwargs)
        store.append(out.cpu().numpy().copy())
        return out
    monkeypatch.setattr(module, name, wrapped)


def check_avi(path, video, fps, quality):
    from dino_tracker_amd import video_out
    from PIL import Image
    assert path.endswith(".avi") and os.path.isfile(path)
    frames, info = video_out.read_mjpeg_avi(path, with_info=True)
    T, H, W = video.shape[:3]
    assert info == {"frames": T, "fps": fps, "width": W, "height": H}
    for data, frame in zip(frames, video):
        assert data == J.encode(frame, quality)
        assert Image.open(io.BytesIO(data)).size == (W, H)


def test_visualize_run_writes_avis(tmp_path, capsys, monkeypatch):
    import viz_data as D
    from dino_tracker_amd import visualize as V
    root = D.write_data_folder(str(tmp_path / "scene"))
    base = ["--data-path", root, "--infer-res-size", "50", "80", "--of-res-size", "50", "80", "--plot-trails", "--fps", "5"]
    rendered = []
    capture(monkeypatch, V, "plot_tracks_v2", rendered)
    capture(monkeypatch, V, "plot_tracks_tails", rendered)
    np.random.seed(0)
    torch.manual_seed(0)
    written = V.main(base + ["--container", "avi", "--quality", "75"])
    said = capsys.readouterr().out
    assert len(written) == 2 and len(rendered) == 2 and said.count("save_video: wrote") == 2 and "Motion-JPEG avi" in said
    assert [os.path.basename(w) for w in written] == ["dotted_tracks_fps_5.avi", "rainbow_fps_5.avi"]
    for path, video in zip(written, rendered):
        assert video.shape == (D.T, D.H, D.W, 3)
        check_avi(path, video, 5, 75)
    # the JPEG folder, and `auto` beside them: what it writes today
    rendered.clear()
    np.random.seed(0)
    torch.manual_seed(0)
    folders = V.main(base[:-3] + ["--fps", "6", "--container", "jpg"])
    assert len(folders) == 1 and os.path.isdir(folders[0]) and sorted(os.listdir(folders[0])) == [f"{i:05d}.jpg" for i in range(D.T)]
    for i, frame in enumerate(rendered[0]):
        with open(os.path.join(folders[0], f"{i:05d}.jpg"), "rb") as fh:
            assert fh.read() == J.encode(frame, 90)
    auto = V.main(base[:-3] + ["--fps", "7"])
    said = capsys.readouterr().out
    assert len(auto) == 1 and os.path.exists(auto[0]) and not auto[0].endswith(".avi")
    if os.path.isdir(auto[0]):
        assert "imageio is not installed" in said and sorted(os.listdir(auto[0])) == [f"{i:05d}.png" for i in range(D.T)]
    else:
        assert auto[0].endswith("dotted_tracks_fps_7.mp4")


def test_pred_vs_gt_writes_avis(tmp_path, capsys, monkeypatch):
    """the data folder of test_gpu_predgt.py::test_cli_writes_the_named_video"""
    from PIL import Image
    from dino_tracker_amd import visualize as V
    gold = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predgt.npz"), allow_pickle=False))
    root = str(tmp_path / "scene")
    video = gold["scene_video"]
    T, H, W = video.shape[:3]
    for sub in ("video", "trajectories", "occlusions"):
        os.makedirs(os.path.join(root, sub))
    for t, frame in enumerate(video):
        Image.fromarray(frame).save(os.path.join(root, "video", f"{t:05d}.png"))
    target = {0: gold["scene_gt"], 3: gold["scene_gt"][:5]}
    occluded = {0: gold["scene_gt_occ"].astype(bool), 3: gold["scene_gt_occ"][:5].astype(bool)}
    with open(os.path.join(root, "bench.pkl"), "wb") as fh:
        pickle.dump({"videos": [{"video_idx": 4, "h": H, "w": W, "target_points": target, "occluded": occluded}]}, fh)
    for f, n in ((0, 8), (3, 5)):
        np.save(os.path.join(root, "trajectories", f"trajectories_{f}.npy"), gold["scene_pred"][:n] * np.float32(2))
        np.save(os.path.join(root, "occlusions", f"occlusion_preds_{f}.npy"), gold["scene_pred_occ"][:n] != 0)
    base = ["pred-vs-gt", "--data-path", root, "--benchmark-pickle-path", os.path.join(root, "bench.pkl"), "--video-id", "4",
            "--infer-res-size", str(2 * H), str(2 * W), "--fps", "2"]
    rendered = []
    capture(monkeypatch, V, "visualize_trajectories_with_gt", rendered)
    np.random.seed(int(gold["scene_seed"]))
    written = V.main(base + ["--container", "avi"])
    said = capsys.readouterr().out
    assert [os.path.basename(w) for w in written] == ["pred_vs_gt_frame_idx_0_fps_2.avi", "pred_vs_gt_frame_idx_3_fps_2.avi"]
    assert said.count("save_video: wrote") == 2 and len(rendered) == 2
    for path, frames in zip(written, rendered):
        assert frames.shape == (T, H, W, 3)
        check_avi(path, frames, 2, 90)
    auto = V.main(base + ["--only-first-frame"])
    assert len(auto) == 1 and os.path.exists(auto[0]) and not auto[0].endswith(".avi")
