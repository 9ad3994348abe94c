"""CPU: the yardstick of the device video ingest.  tests/resize_ref.py restates Pillow's 8-bit LANCZOS resize in numpy; here it is
held against live Pillow (where installed) and against Pillow's committed outputs (tests/golden/resize_lanczos.npz, which needs no
Pillow), video_io.lanczos_tables is held against the restatement's tables, and the new entry points' argument errors are checked
without touching a device.  Integer arithmetic throughout: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

import resize_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_lanczos.npz")
# beyond the shared cases: the pipeline's own shapes and an up-scale, against live Pillow only
LIVE_ONLY = ((480, 854, 476, 854), (1080, 1920, 476, 854), (100, 100, 333, 217))
SIZE_PAIRS = ((53, 24), (24, 53), (300, 7), (400, 3), (1, 9), (7, 1), (5, 1), (29, 13), (480, 476), (1920, 854), (1080, 476), (64, 64))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def pillow_resize(frames, h, w):
    from PIL import Image
    out = []
    for f in frames:
        img = Image.fromarray(f[:, :, 0] if f.shape[2] == 1 else f)
        out.append(np.asarray(img.resize((w, h), Image.LANCZOS)).reshape(h, w, f.shape[2]))
    return np.stack(out)


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_restatement_equals_live_pillow(case, content):
    pytest.importorskip("PIL")
    name, N, H, W, C, h, w = case
    x = R.case_input(name, content)
    assert np.array_equal(R.resize(x, h, w), pillow_resize(x, h, w))


@pytest.mark.parametrize("shape", LIVE_ONLY, ids=["x".join(map(str, s)) for s in LIVE_ONLY])
def test_restatement_equals_live_pillow_at_pipeline_sizes(shape):
    pytest.importorskip("PIL")
    H, W, h, w = shape
    x = np.random.default_rng(H).integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)
    assert np.array_equal(R.resize(x, h, w), pillow_resize(x, h, w))


def test_restatement_equals_goldens(gold):
    """Pillow's committed outputs, regenerated inputs: no Pillow needed.  Both clamps are reached by the {0, 255} content."""
    assert len(gold.files) == 1 + len(R.all_cases())
    below = above = False
    for (name, N, H, W, C, h, w), content in R.all_cases():
        x = R.case_input(name, content)
        want = gold[f"{name}/{content}"]
        assert want.shape == (N, h, w, C) and want.dtype == np.uint8
        assert np.array_equal(R.resize(x, h, w), want), (name, content)
        if content == "binary" and W != w:   # the accumulator of the first pass, before the clamp
            k, b = R.tables(W, w)
            idx = np.minimum(b[:, :1] + np.arange(k.shape[1])[None], W - 1)
            acc = (1 << 21) + (x.astype(np.int64).transpose(0, 1, 3, 2)[..., idx] * k).sum(-1)
            below, above = below or bool((acc < 0).any()), above or bool((acc >> 22 > 255).any())
    assert below and above


def test_frames_of_a_batch_are_independent():
    x = R.case_input("frames3", "uniform")
    whole = R.resize(x, 16, 24)
    assert not np.array_equal(x[0], x[1])
    for n in range(3):
        assert np.array_equal(whole[n:n + 1], R.resize(x[n:n + 1], 16, 24))


@pytest.mark.parametrize("pair", SIZE_PAIRS, ids=[f"{a}-{b}" for a, b in SIZE_PAIRS])
def test_lanczos_tables_equal_the_restatement(pair):
    from dino_tracker_amd import video_io
    k, b = video_io.lanczos_tables(*pair)
    rk, rb = R.tables(*pair)
    assert k.dtype == np.int32 and b.dtype == np.int32 and not k.flags.writeable
    assert np.array_equal(k, rk) and np.array_equal(b, rb)
    scale = pair[0] / pair[1]
    assert k.shape == (pair[1], 2 * int(np.ceil(3 * max(scale, 1.0))) + 1)
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= pair[0]).all() and (b[:, 1] >= 1).all() and (b[:, 1] <= k.shape[1]).all()
    # what the kernels rely on: exact 24-bit products, no int32 overflow of a row, nothing beyond a row's count
    assert np.abs(k).max() < (1 << 23)
    assert (255 * np.abs(k.astype(np.int64)).sum(axis=1) + (1 << 21)).max() < (1 << 31)
    assert not (k * (np.arange(k.shape[1])[None] >= b[:, 1:])).any()
    assert video_io.lanczos_tables(*pair)[0] is k   # cached per size pair


def test_lanczos_tables_refuse_bad_sizes():
    from dino_tracker_amd import video_io
    for pair in ((0, 4), (4, 0), (-3, 2)):
        with pytest.raises(ValueError):
            video_io.lanczos_tables(*pair)


def test_python_entry_points_refuse_without_a_device():
    """No CPU fallback, and the shape / dtype / option errors come before any device call."""
    from dino_tracker_amd import train, video_io
    u8 = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video_io.resize_lanczos(u8, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video_io.resize_tensor_frames_lanczos(torch.zeros((2, 3, 8, 8)), 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video_io.load_video("nowhere", resize=(4, 4), device="cpu")
    with pytest.raises(ValueError, match="out must be"):
        video_io.resize_lanczos(u8, 4, 4, out="f16")
    import inspect
    assert inspect.signature(train.load_video).parameters["device"].default is None


def test_c_entry_points_validate_before_any_device_call():
    """dtk_resize_u8 returns -1 with a message for every refused argument; the pointers are dummies that are never read."""
    import __graft_entry__ as entry
    from dino_tracker_amd import _lib, ops
    entry.build()
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(N=1, H=8, W=8, C=3, h=4, w=4, ksx=7, ksy=7, form=0, opts=0, inp=p, out=p, kx=p, bx=p, ky=p, by=p, lut=p):
        rc = lib.dtk_resize_u8(inp, N, H, W, C, h, w, kx, bx, ksx, ky, by, ksy, lut, form, opts, out, None, 0, None)
        return rc, lib.dtk_last_error()

    for kwargs, message in ((dict(C=2), b"C must be 1 or 3"), (dict(C=4), b"C must be 1 or 3"), (dict(N=0), b"sizes must be positive"),
                            (dict(H=0), b"sizes must be positive"), (dict(W=-1), b"sizes must be positive"),
                            (dict(h=0), b"sizes must be positive"), (dict(w=0), b"sizes must be positive"),
                            (dict(form=2), b"out_form"), (dict(form=-1), b"out_form"), (dict(opts=2), b"unknown option bits 0x2"),
                            (dict(opts=5), b"unknown option bits 0x4"), (dict(inp=None), b"null pointer"), (dict(out=None), b"null pointer"),
                            (dict(form=1, lut=None), b"null pointer"), (dict(kx=None), b"null pointer"), (dict(bx=None), b"null pointer"),
                            (dict(ky=None), b"null pointer"), (dict(by=None), b"null pointer"), (dict(ksx=0), b"ksize must be >= 1"),
                            (dict(ksy=0), b"ksize must be >= 1")):
        rc, err = call(**kwargs)
        assert rc == -1 and message in err, (kwargs, rc, err)
    # the general form without its workspace is refused too, still before any launch
    rc, err = call(opts=ops.RESIZE_FORCE_GENERAL)
    assert rc == -1 and b"workspace of 96 bytes" in err, err
    # dtk_resize_workspace_bytes: 0 for what dtk_resize_u8 refuses, for a skipped pass and for the fused form
    ws = lib.dtk_resize_workspace_bytes
    assert ws(1, 8, 8, 2, 4, 4, 7, 0) == 0 and ws(1, 8, 8, 3, 4, 4, 7, 2) == 0 and ws(1, 8, 8, 3, 4, 4, 0, 0) == 0
    assert ws(2, 8, 8, 3, 4, 4, 7, 0) == 0 and ws(2, 8, 8, 3, 4, 4, 7, 1) == 2 * 8 * 4 * 3
    assert ws(2, 8, 8, 3, 8, 4, 7, 1) == 0 and ws(2, 8, 8, 3, 4, 8, 7, 1) == 0
    assert ws(1, 400, 8, 3, 3, 5, 801, 0) == 400 * 5 * 3   # the rows of one tile exceed 64 KiB of LDS


def test_constants_match_header():
    import re
    from dino_tracker_amd import ops
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dtk.h")).read()
    for name, value in (("DTK_RESIZE_OUT_U8_HWC", ops.RESIZE_OUT_U8_HWC), ("DTK_RESIZE_OUT_F32_CHW", ops.RESIZE_OUT_F32_CHW),
                        ("DTK_RESIZE_FORCE_GENERAL", ops.RESIZE_FORCE_GENERAL), ("DTK_RESIZE_TILE_H", ops.RESIZE_TILE_H),
                        ("DTK_RESIZE_TILE_W", ops.RESIZE_TILE_W)):
        m = re.search(rf"#define {name} (\d+)", text)
        assert m and int(m.group(1)) == value, name


def test_byte_round_trip_through_float():
    """ToTensor then ToPILImage: v / 255 * 255 in fp32 truncates back to v for every byte, so frames that came from bytes lose nothing
    in resize_tensor_frames_lanczos' quantisation (a value just below a step still truncates down)."""
    v = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(v.float().div(255).mul(255).to(torch.uint8), v)
    assert torch.tensor([254.999 / 255]).mul(255).to(torch.uint8).item() == 254
