"""-m gpu: the fp16 operand mode of the Delta-DINO refinement (DTK_DD_FP16: first layer fused with its blur-pool) against the
kernel sequence it replaced (DTK_DD_FP16_V1), bit for bit.  No oracle: two modes of the library on the inputs of
tests/test_gpu_p2.py (synth seeds 61 / 62 / 63).  Almost every intermediate pixel feeds a sampled layer-4 cell, so equality of
the refined volume checks all four stages."""
import pytest
import torch

from dino_tracker_amd import ops, synth
from oracle import ref_algo as A

pytestmark = pytest.mark.gpu

DD_FRAME_BATCH = 8  # csrc/delta_dino.hip

# C, H, W, T
GEOMETRIES = [
    (32, 57, 71, 2),     # odd in both dimensions, 57 -> 29 -> 15 -> 8 through the pools; layer 4 smaller than one tile
    (32, 99, 127, 2),    # odd sizes
    (32, 30, 44, 2),     # maps smaller than a halo: reflect()'s clamp
    (32, 98, 126, 9),    # crosses DD_FRAME_BATCH: a full chunk and a 1-frame chunk
    (384, 101, 131, 2),  # six 64-wide cout tiles; partial pixel tiles on both edges
    (32, 143, 211, 2),   # several tiles per dimension with partial last ones (two row segments, four column bands in layer 1)
]


def _inputs(C, H, W, T):
    ph, pw = A.feature_grid(H, W)
    return (synth.synth_video(T, H, W, seed=61), synth.synth_features(T, C, ph, pw, seed=62),
            synth.synth_delta_dino_weights(C, seed=63))


def _refined(video, dino, delta, mode, profile=False):
    from gpu_util import make_tracker
    trk = make_tracker(video, dino, synth.synth_head_weights(3), delta=delta, p2_operands=mode)
    trk.eval()
    prof = None
    if profile:
        ops.profile_enable(True)
    try:
        trk.cache_refined_embeddings()
        if profile:
            prof = ops.profile_collect()
    finally:
        if profile:
            ops.profile_enable(False)
    _, norms, _ = trk.features()
    return trk.refined_features.cpu(), norms.cpu(), prof


@pytest.mark.parametrize("C,H,W,T", GEOMETRIES)
def test_fp16_equals_fp16_v1_bitwise(C, H, W, T):
    video, dino, delta = _inputs(C, H, W, T)
    new, new_norms, _ = _refined(video, dino, delta, "fp16")
    old, old_norms, _ = _refined(video, dino, delta, "fp16_v1")
    assert new.shape == old.shape and torch.isfinite(old).all()
    assert (old - dino).abs().mean() > 1e-3   # the residual is there
    assert torch.equal(new, old), f"max |fp16 - fp16_v1| = {(new - old).abs().max().item():.3g}"
    assert torch.equal(new_norms, old_norms)


def test_modes_run_different_kernels():
    """Liveness: the equality above does not hold because both modes run the same code.  dd_blurpool launches per frame chunk:
    three in the replaced sequence, two once the first blur-pool is inside dd_conv1."""
    C, H, W, T = 32, 98, 126, 9
    chunks = -(-T // DD_FRAME_BATCH)
    video, dino, delta = _inputs(C, H, W, T)
    for mode, per_chunk in (("fp16_v1", 3), ("fp16", 2)):
        _, _, prof = _refined(video, dino, delta, mode, profile=True)
        assert prof["dd_blurpool"][1] == per_chunk * chunks, (mode, prof["dd_blurpool"])
        assert prof["dd_conv1"][1] == chunks, (mode, prof["dd_conv1"])

