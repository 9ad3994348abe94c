"""CPU: the reference that the ViT-g/14 GPU tests are judged by (tests/vitg_ref.py) is itself checked --
(i) the restated SwiGLU block against transformers' Dinov2 layer with use_swiglu_ffn, (ii) an fp32 emulation of a correct w12 kernel
passes the per-element bound, (iii) four planted defects fail it, (iv) the device's silu expression in fp32 stays within the error its
source comment states, (v) the seeded weights of ViT-S / B / L are bit for bit what they were before ViT-g joined synth.VIT_CONFIGS."""
import hashlib

import pytest
import torch

import vit_gemm_ref as R
import vitg_ref as G
from dino_tracker_amd import synth

F16, BF16 = torch.float16, torch.bfloat16


def test_block_matches_transformers_swiglu_layer():
    """(i) tests/hf_swiglu_crosscheck.py: vitg_ref.vitg_block in float64 vs transformers' Dinov2 layer with Dinov2SwiGLUFFN, random
    weights mapped across, to 1e-4.  In a clean interpreter, as tests/test_oracle_vs_reference.py runs its cross-check: the torchvision
    shim that other tests install for the reference must not be visible to transformers."""
    import os
    import subprocess
    import sys
    pytest.importorskip("transformers")
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hf_swiglu_crosscheck.py")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr


def test_pack_index_is_the_documented_interleave():
    idx = G.pack_index()
    assert sorted(idx.tolist()) == list(range(2 * G.HIDDEN))
    for g in (0, 1, 127):
        assert idx[64 * g:64 * g + 32].tolist() == list(range(32 * g, 32 * g + 32))
        assert idx[64 * g + 32:64 * g + 64].tolist() == list(range(G.HIDDEN + 32 * g, G.HIDDEN + 32 * g + 32))


@pytest.mark.parametrize("split", [False, True], ids=["fast", "split"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_emulated_kernel_passes_and_defects_fail(dtype, split):
    """(ii) + (iii) on 48 rows: the worst |got - ref| / bound of the correct emulation is printed; every defect must exceed 1."""
    o = G.make_fc1(48, dtype, 11 + split, split=split)
    worst, at = G.check(o, G.emulate_fc1(o))
    print(f"vitg fc1 emulation {dtype} split={split}: worst |got - ref| / bound = {worst:.3f} at {at}")
    for d in ("silu_on_value", "no_bias_value", "pair_shift"):
        with pytest.raises(AssertionError, match="bound"):
            G.check(o, G.emulate_fc1(o, defect=d))
    o2 = G.make_fc2(48, dtype, 5, split=split)
    got = R.emulate(o2)
    worst, _ = G.check(o2, got)
    print(f"vitg w3 emulation {dtype} split={split}: worst |got - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_fourth_product_fails_the_exact_sum_class(dtype):
    """A lo x lo product brings a realistic result CLOSER to float64 on the full operands, so no realistic bound can reject it; with
    integer planes the three-product sum is exact and the fourth product shows (as tests/test_vit_gemm_reference.py does for GELU-free
    roles).  The correct emulation passes the same check."""
    o = G.make_fc1(48, dtype, 12, split=True, exact_sums=True)
    worst, _ = G.check(o, G.emulate_fc1(o))
    print(f"vitg fc1 exact-sum emulation {dtype}: worst |got - ref| / bound = {worst:.3f}")
    with pytest.raises(AssertionError, match="bound"):
        G.check(o, G.emulate_fc1(o, defect="lolo"))


def test_device_silu_expression_within_its_stated_error():
    assert G.g_silu_from_source() == G.G_SILU
    v = torch.cat([torch.linspace(-100.0, 100.0, 2_000_001, dtype=torch.float64), torch.tensor([-1e4, 1e4], dtype=torch.float64),
                   torch.tensor([-3.4e38, -88.8, -87.0, -0.0, 0.0, 3.4e38], dtype=torch.float64)]).float()
    got = G.silu_device_f32(v)
    assert bool(torch.isfinite(got).all())
    assert float(got[-6]) == 0.0 and float(got[v == -1e4][0]) == 0.0          # the very negative tail: a zero, not NaN
    err = (got.double() - G.silu64(v.double())).abs() / v.double().abs().clamp(min=1.0)
    print(f"device silu expression in fp32: max |err| / max(1, |v|) = {float(err.max()):.3e} (stated {G.G_SILU:.1e})")
    assert float(err.max()) <= G.G_SILU


PARENT_HASHES = {   # sha256 over sorted(name, tensor bytes) of make_vit_weights(name, seed=2), recorded before ViT-g was added
    "dinov2_vits14": "b8666e34730bbd7bd59ae50bc929a73aa9a621164ad077e6b3d3cd10175484d9",
    "dinov2_vitb14": "29b3ddc283c8482ea0736a2b5accebb21c8336bff299aaf0b28dea2322fa6449",
    "dinov2_vitl14": "13f85a207815c37f081cdbd7bb7a60109c183821d67b06774f1c55658c8f4d63",
}


@pytest.mark.parametrize("name", list(PARENT_HASHES))
def test_seeded_weights_of_the_other_models_are_unchanged(name):
    sd = synth.make_vit_weights(name, seed=2)
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    assert h.hexdigest() == PARENT_HASHES[name]


def test_vitg_weights_and_truncation():
    cfg = synth.VIT_CONFIGS["dinov2_vitg14"]
    assert cfg == dict(dim=1536, depth=40, heads=24, ffn="swiglu", hidden=4096)
    sd = synth.make_vit_weights("dinov2_vitg14", seed=5, nblocks=1)
    assert sd["blocks.0.mlp.w12.weight"].shape == (8192, 1536) and sd["blocks.0.mlp.w3.weight"].shape == (1536, 4096)
    assert "blocks.1.norm1.weight" not in sd and "blocks.0.mlp.fc1.weight" not in sd
    full = synth.make_vit_weights("dinov2_vits14", seed=5)
    part = synth.make_vit_weights("dinov2_vits14", seed=5, nblocks=2)
    assert all(torch.equal(full[k], v) for k, v in part.items()) and "blocks.2.norm1.weight" not in part
