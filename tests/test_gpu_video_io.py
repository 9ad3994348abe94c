"""GPU: the device video ingest (csrc/resize.hip, dino_tracker_amd/video_io.py) against the numpy restatement of Pillow's 8-bit
LANCZOS resize (tests/resize_ref.py) and Pillow's own committed outputs (tests/golden/resize_lanczos.npz).  The operation is integer
arithmetic, so every comparison is torch.equal: zero differing bytes, no tolerance anywhere.

The cases (resize_ref.CASES, H x W -> h x w; the kernel's tile is 32 x 64 output pixels, ops.RESIZE_TILE_H / _W):
  down_rgb   37x53 -> 16x24   non-integer down-scale on both axes, ksize 15, rows of 159 bytes (no multiple of 4)
  up_rgb     16x24 -> 37x53   up-scale, support 3
  v_only     40x64 -> 36x64   horizontal pass skipped: the pipeline's own 480 -> 476 in small
  h_only     40x64 -> 40x31   vertical pass skipped
  ksize259   20x300 -> 19x7   259 horizontal taps
  to_1x1 / from_1x1           degenerate sizes
  mode_l     41x29 -> 17x13   C = 1
  frames3    37x53 -> 16x24   N = 3 distinct frames: frame strides
  multi_tile 70x131 -> 45x83  two tiles on both axes, the second ragged on both
  tall       400x8 -> 3x5     the rows of one tile do not fit in LDS: the entry point leaves the fused form on its own
  same_size  12x10 -> 12x10   both passes skipped: a change of form only
each on uniform random bytes and on random {0, 255} pixels (the accumulator passes both clamps), in both output forms and in both
kernel forms (picked by the entry point, and forced general)."""
import os

import numpy as np
import pytest
import torch

import resize_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_lanczos.npz")


@pytest.fixture(scope="module")
def refs():
    """(case, content) -> (input uint8 [N, H, W, C], restatement output uint8 [N, h, w, C]); computed once, read-only, and equal to
    Pillow's committed outputs."""
    gold = np.load(GOLD)
    out = {}
    for (name, N, H, W, C, h, w), content in R.all_cases():
        x = R.case_input(name, content)
        y = R.resize(x, h, w)
        assert np.array_equal(y, gold[f"{name}/{content}"]), (name, content)
        x.setflags(write=False)
        y.setflags(write=False)
        out[name, content] = (x, y)
    return out


def differing(a: torch.Tensor, b: torch.Tensor) -> int:
    return int((a != b).sum().item()) if a.shape == b.shape else -1


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_resize_equals_pillow(case, content, refs):
    from dino_tracker_amd import video_io
    name, N, H, W, C, h, w = case
    x, y = refs[name, content]
    xd = torch.from_numpy(x.copy()).to(DEV)
    want_u8 = torch.from_numpy(y.copy())
    want_f32 = torch.from_numpy(R.to_tensor(y))
    assert torch.equal(want_f32, want_u8.permute(0, 3, 1, 2).float().div(255))   # the restatement's ToTensor is torch's
    for general in (False, True):
        got_u8 = video_io.resize_lanczos(xd, h, w, out="u8", force_general=general).cpu()
        got_f32 = video_io.resize_lanczos(xd, h, w, out="f32", force_general=general).cpu()
        print(name, content, "general" if general else "picked", "differing: u8", differing(got_u8, want_u8), "f32",
              differing(got_f32, want_f32))
        assert got_u8.dtype == torch.uint8 and torch.equal(got_u8, want_u8), (name, content, general)
        assert got_f32.dtype == torch.float32 and torch.equal(got_f32, want_f32), (name, content, general)
    if N == 1:   # the [H, W, C] form of the argument
        assert torch.equal(video_io.resize_lanczos(xd[0], h, w).cpu(), want_u8[0])


def test_form_selection():
    """The entry point's choice, seen through the workspace it asks for: only `tall` leaves the fused form on its own (400 rows of
    192 bytes are more than 64 KiB of LDS); forcing the general form asks for the intermediate wherever both passes run."""
    from dino_tracker_amd import ops, video_io
    for name, N, H, W, C, h, w in R.CASES:
        ksy = video_io.lanczos_tables(H, h)[0].shape[1]
        picked = ops.resize_workspace_bytes(N, H, W, C, h, w, ksy)
        forced = ops.resize_workspace_bytes(N, H, W, C, h, w, ksy, ops.RESIZE_FORCE_GENERAL)
        two_pass = H != h and W != w
        assert picked == (N * H * w * C if name == "tall" else 0), name
        assert forced == (N * H * w * C if two_pass else 0), name


def test_float_frames_twin():
    """resize_tensor_frames_lanczos (data/data_utils.py:47-52): float frames quantised as ToPILImage does -- mul(255) in fp32, then
    truncation, whatever that gives for a value -- against the same quantisation by torch on the CPU followed by the restatement.
    The input holds v / 255 for all 256 v, exact 0 and 1, a value just below an integer step, and random floats."""
    from dino_tracker_amd import video_io
    g = torch.Generator().manual_seed(7)
    frames = torch.rand((2, 3, 16, 24), generator=g)
    ramp = torch.arange(256, dtype=torch.float32).div(255)
    frames[0, 0].view(-1)[:256] = ramp
    frames[1, 2].view(-1)[100:356] = ramp.flip(0)
    frames[0, 1, 0, :4] = torch.tensor([0.0, 1.0, 0.5, 254.999 / 255])
    q = frames.mul(255).to(torch.uint8)
    assert q[0, 1, 0, 3] == 254 and len(torch.unique(q)) == 256   # truncation, not rounding; every byte value occurs
    want = torch.from_numpy(R.to_tensor(R.resize(q.permute(0, 2, 3, 1).contiguous().numpy(), 37, 53)))
    got = video_io.resize_tensor_frames_lanczos(frames.to(DEV), 37, 53)
    assert got.is_cuda and got.dtype == torch.float32
    print("float twin differing:", differing(got.cpu(), want))
    assert torch.equal(got.cpu(), want)
    one = video_io.resize_tensor_frames_lanczos(frames[:, :1].contiguous().to(DEV), 9, 31)   # ToPILImage of one channel: mode L
    assert torch.equal(one.cpu(), torch.from_numpy(R.to_tensor(R.resize(q[:, :1].permute(0, 2, 3, 1).contiguous().numpy(), 9, 31))))


def _write_frames(folder, frames, mode):
    from PIL import Image
    folder.mkdir()
    for t, f in enumerate(frames):
        ext = "png" if t % 2 == 0 else "jpg"   # both globs; the order is by name across them
        img = Image.fromarray(f[:, :, 0] if mode == "L" else f)
        img.save(str(folder / f"{t:05d}.{ext}"), **({"quality": 95} if ext == "jpg" else {}))
    return str(folder)


def _host_expected(folder, resize):
    """What the host path gives.  RGB: train.load_video itself.  Mode L: the reference's load_video (Image.resize + ToTensor ->
    [T, 1, h, w]); the host train.load_video cannot load a mode-L folder (its permute wants three axes)."""
    from PIL import Image
    from dino_tracker_amd import train, video_io
    files = video_io.video_files(folder)
    if Image.open(str(files[0])).mode != "L":
        return train.load_video(folder, resize=resize)
    with pytest.raises(RuntimeError):
        train.load_video(folder, resize=resize)
    frames = [np.asarray(Image.open(str(f)).resize((resize[1], resize[0]), Image.LANCZOS)) for f in files]
    return torch.from_numpy(np.stack(frames))[:, None].float().div(255)


@pytest.mark.parametrize("mode", ("RGB", "L"))
@pytest.mark.parametrize("shape", ((40, 64, 36, 64), (37, 53, 16, 24)), ids=("40x64-36x64", "37x53-16x24"))
def test_load_video_end_to_end(tmp_path, shape, mode):
    """A folder of frames through video_io.load_video on the device against the host path, bit for bit; train.load_video's
    `device=` is the same path."""
    pytest.importorskip("PIL")
    from dino_tracker_amd import train, video_io
    H, W, h, w = shape
    rng = np.random.default_rng([H, W, len(mode)])
    folder = _write_frames(tmp_path / "video", rng.integers(0, 256, size=(3, H, W, 3), dtype=np.uint8), mode)
    want = _host_expected(folder, (h, w))
    got = video_io.load_video(folder, resize=(h, w), device=DEV)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, len(mode), h, w)
    print(shape, mode, "differing:", differing(got.cpu(), want))
    assert torch.equal(got.cpu(), want)
    routed = train.load_video(folder, resize=(h, w), device=DEV)
    assert routed.is_cuda and torch.equal(routed, got)
    assert torch.equal(video_io.load_video(folder, resize=(h, w), num_frames=2, device=DEV), got[:2])
    if mode == "RGB":   # no resize: ToTensor alone
        assert torch.equal(video_io.load_video(folder, device=DEV).cpu(), train.load_video(folder))


def test_load_video_mixed_sizes_take_the_host_path(tmp_path):
    """Frames of different sizes still load: through the host code, uploaded afterwards."""
    pytest.importorskip("PIL")
    from PIL import Image
    from dino_tracker_amd import train, video_io
    rng = np.random.default_rng(3)
    folder = tmp_path / "mixed"
    folder.mkdir()
    for t, (H, W) in enumerate(((37, 53), (40, 64), (37, 53))):
        Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(str(folder / f"{t:05d}.png"))
    assert video_io._decode_pinned(video_io.video_files(folder)) is None
    got = video_io.load_video(str(folder), resize=(16, 24), device=DEV)
    assert got.is_cuda and torch.equal(got.cpu(), train.load_video(str(folder), resize=(16, 24)))
