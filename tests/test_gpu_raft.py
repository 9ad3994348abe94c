"""GPU: RaftLarge.flow (dtk_raft_forward) against the float64 restatement of tests/raft_ref.py on the seeded weights, under the
flow-trajectory tests' tolerance policy (docs/PARITY.md):

* ref_dev = max |float32 restatement - float64 restatement| on the same inputs, computed here;
* split operands: the device lies within 4 x ref_dev of float64 (the factor allows for the device's different summation order);
* fp16 operands: within 4 x the deviation of the fp16-rounding emulation (every convolution / correlation operand rounded to
  fp16, in float64) from float64.

The reference passes (float64, float32, fp16 emulation) run once per image size on three pairs -- a pair both ways plus a third
pair -- and return the predictions after 1, 2 and 24 updates; the batch of two is the first two pairs (every stage of the network
is per sample, so the batch of three's reference restricted to them IS the batch of two's).
"""
import os

import pytest
import torch

import raft_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UPDATES = (1, 2, 24)
SIZES = ((128, 136), (136, 128))


@pytest.fixture(scope="module")
def weights():
    from dino_tracker_amd import synth
    return synth.make_raft_weights(0)


@pytest.fixture(scope="module")
def models(weights):
    from dino_tracker_amd.raft import RaftLarge
    return {m: RaftLarge(weights, DEV, operands=m) for m in ("split", "fp16")}


_refs = {}


def images(H, W):
    a, b = R.make_images(2, H, W, seed=H)
    return torch.cat((a[:1], b[:1], a[1:])), torch.cat((b[:1], a[:1], b[1:]))      # a pair both ways, then a third pair


def reference(weights, H, W):
    """computed once per size and never modified: {updates: (float64 flow, ref_dev, fp16 emulation deviation)}"""
    if (H, W) not in _refs:
        from dino_tracker_amd.raft import fold_batchnorm
        src, dst = images(H, W)
        f64 = R.raft_forward(weights, src, dst, 24, torch.float64, return_at=UPDATES)
        f32 = R.raft_forward(weights, src, dst, 24, torch.float32, return_at=UPDATES)
        f16 = R.raft_forward(fold_batchnorm(weights), src, dst, 24, torch.float64, rnd=R.fp16_round, return_at=UPDATES)
        _refs[H, W] = {k: (f64[k], (f32[k].double() - f64[k]).abs().amax(dim=(1, 2, 3)), (f16[k] - f64[k]).abs().amax(dim=(1, 2, 3)))
                       for k in UPDATES}
    return _refs[H, W]


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("batch", [2, 3])
@pytest.mark.parametrize("mode", ["split", "fp16"])
def test_flow_against_float64(weights, models, H, W, batch, mode):
    src, dst = images(H, W)
    ref = reference(weights, H, W)
    for k in UPDATES:
        f64, ref_dev, f16_dev = ref[k]
        got = models[mode].flow(src[:batch].to(DEV), dst[:batch].to(DEV), num_flow_updates=k).double().cpu()
        assert got.shape == (batch, 2, H, W)
        err = (got - f64[:batch]).abs().amax(dim=(1, 2, 3))
        yard = (ref_dev if mode == "split" else f16_dev)[:batch]
        print(f"raft {H}x{W} batch {batch} {mode} updates {k}: max |flow| {f64[:batch].abs().max().item():.2f} px, device err "
              f"{err.tolist()}, yardstick {yard.tolist()} (x 4 allowed)")
        assert bool((err <= 4 * yard).all()), (k, err.tolist(), yard.tolist())


def test_flow_fn_pads_and_crops(weights, models):
    """131 x 141 frames in [0, 1]: padded to 136 x 144 (replicate), mapped to [-1, 1], the flow cropped back."""
    from dino_tracker_amd import synth
    from dino_tracker_amd.raft import raft_flow_fn
    v = synth.synth_video(2, 131, 141, seed=8, vx=2.5, vy=1.5)
    src, dst = v[:1], v[1:]
    f64 = R.raft_flow_fn_ref(weights, 4, torch.float64)(src, dst)
    f32 = R.raft_flow_fn_ref(weights, 4, torch.float32)(src, dst)
    ref_dev = (f32.double() - f64).abs().max().item()
    got = raft_flow_fn(models["split"], 4)(src.to(DEV), dst.to(DEV))
    assert got.shape == (1, 2, 131, 141) and got.is_contiguous()
    err = (got.double().cpu() - f64).abs().max().item()
    print(f"raft_flow_fn 131x141: device err {err:.3e}, ref_dev {ref_dev:.3e}")
    assert err <= 4 * ref_dev


def test_refusals_leave_the_output_untouched(models):
    import ctypes
    from dino_tracker_amd import _lib
    m = models["split"]
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def call(N, H, W, img=None, out=None, ws=None, ws_bytes=None, updates=2):
        img = torch.zeros(N, 3, H, W, device=DEV) if img is None else img
        need = max(int(L.dtk_raft_workspace_bytes(N, H, W)), int(L.dtk_raft_workspace_bytes(1, 128, 128)))
        ws_t = torch.empty(need, dtype=torch.uint8, device=DEV)
        return L.dtk_raft_forward(ctypes.byref(m.model), img.data_ptr() if hasattr(img, "data_ptr") else img, img.data_ptr()
                                  if hasattr(img, "data_ptr") else img, N, H, W, updates, m.mode, out.data_ptr(),
                                  ws_t.data_ptr() if ws is None else ws, need if ws_bytes is None else ws_bytes, stream)

    out = torch.full((1, 2, 136, 136), 3.5, device=DEV)
    assert call(1, 132, 136, out=out) == -1 and b"divisible by 8" in L.dtk_last_error()          # not divisible by 8
    assert call(1, 120, 136, out=out) == -1 and b"16 x 16" in L.dtk_last_error()                 # a 15 x 17 feature map
    assert call(1, 136, 136, out=out, ws_bytes=1024) == -3                                       # a short workspace
    host = (ctypes.c_float * (3 * 136 * 136))()
    assert call(1, 136, 136, img=ctypes.addressof(host), out=out) == -1 and b"host" in L.dtk_last_error()
    assert call(1, 136, 136, out=out, updates=0) == -1
    assert L.dtk_raft_workspace_bytes(1, 132, 136) == 0 and L.dtk_raft_workspace_bytes(1, 120, 136) == 0
    torch.cuda.synchronize()
    assert bool((out == 3.5).all())
    with pytest.raises(ValueError, match="divisible by 8"):
        m.flow(torch.zeros(1, 3, 132, 136), torch.zeros(1, 3, 132, 136))
    with pytest.raises(ValueError, match="16 x 16"):
        m.flow(torch.zeros(1, 3, 120, 136), torch.zeros(1, 3, 120, 136))


def test_flow_trajectories_run_uses_the_device_raft(weights, models, tmp_path):
    """flow_trajectories.run(raft_weights=...) on three PNG frames writes exactly chain_trajectories of the flows RaftLarge.flow
    returns for those frames: the plumbing (loading, padding, batching both ways, chaining), not a threshold decision across
    arithmetics.  The seeded network's forward and backward flows are not cycle-consistent to a pixel, so the threshold is 1e4 px:
    every pixel the forward warp hits starts a trajectory, and the tensor compared is not empty."""
    import numpy as np
    from PIL import Image
    from dino_tracker_amd import flow_trajectories as FT
    from dino_tracker_amd import synth
    from dino_tracker_amd.raft import raft_flow_fn
    from dino_tracker_amd.train import load_video
    frames = tmp_path / "video"
    frames.mkdir()
    v = synth.synth_video(3, 128, 136, seed=12, vx=1.5, vy=0.5)
    for i, f in enumerate(v):
        Image.fromarray((f.permute(1, 2, 0).numpy() * 255 + 0.5).astype(np.uint8)).save(frames / f"{i:05d}.png")
    wpath = tmp_path / "raft.pt"
    torch.save(weights, wpath)
    out = tmp_path / "traj" / "trajectories.pt"
    traj = FT.run(str(frames), str(out), threshold=1e4, device=DEV, raft_weights=str(wpath))
    video = load_video(str(frames), device=DEV)
    fn = raft_flow_fn(models["split"])
    pairs = [fn(torch.stack((video[i], video[i + 1])), torch.stack((video[i + 1], video[i]))) for i in range(2)]
    want = FT.chain_trajectories(torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs]), threshold=1e4, device=DEV).cpu()
    saved = torch.load(out)
    assert traj.shape == want.shape and traj.shape[1:] == (3, 2) and traj.shape[0] > 100
    assert torch.equal(torch.nan_to_num(traj, nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    assert torch.equal(torch.nan_to_num(saved, nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    # the environment variable selects the same network
    os.environ["DTK_RAFT_WEIGHTS"] = str(wpath)
    try:
        again = FT.run(str(frames), str(tmp_path / "t2.pt"), threshold=1e4, device=DEV)
    finally:
        del os.environ["DTK_RAFT_WEIGHTS"]
    assert torch.equal(torch.nan_to_num(again, nan=-1.0), torch.nan_to_num(want, nan=-1.0))
