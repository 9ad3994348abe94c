"""CPU: the premises of the RAFT tests.  tests/raft_ref.py is the yardstick of tests/test_gpu_raft*.py; here:

* the tolerance policy's premise on the seeded weights: the float32 restatement stays below 1e-3 px of the float64 one at
  128 x 136 after 24 updates (measured: 2.2e-5 px on a flow of 29 px), so "4 x ref_dev" is a sharp bound;
* the 16 x 16 minimum raises;
* the comparison rejects one planted defect at a time: each moves the flow by far more than 4 x ref_dev;
* the loader is strict and synth.make_raft_weights uses the documented naming.
"""
import pytest
import torch

import raft_ref as R
from dino_tracker_amd import raft, synth

H, W, UPDATES = 128, 136, 24


@pytest.fixture(scope="module")
def weights():
    return synth.make_raft_weights(0)


@pytest.fixture(scope="module")
def pair():
    a, b = R.make_images(1, H, W, seed=5)
    return a, b


@pytest.fixture(scope="module")
def f64(weights, pair):
    return R.raft_forward(weights, *pair, UPDATES, torch.float64)


@pytest.fixture(scope="module")
def ref_dev(weights, pair, f64):
    return (R.raft_forward(weights, *pair, UPDATES, torch.float32).double() - f64).abs().max().item()


def test_policy_premise(f64, ref_dev):
    print(f"max |flow| {f64.abs().max().item():.2f} px, ref_dev {ref_dev:.3e} px")
    assert f64.shape == (1, 2, H, W)
    assert 1.0 < f64.abs().max().item() < 100.0      # the scaled network moves, and is not chaotic
    assert ref_dev < 1e-3


def test_folding_batchnorm_changes_nothing(weights, pair, f64):
    folded = raft.fold_batchnorm(weights)
    assert not any("running" in k or "num_batches" in k for k in folded) and len(folded) == 2 * 47
    assert (R.raft_forward(folded, *pair, UPDATES, torch.float64) - f64).abs().max().item() < 1e-9


def test_fp16_emulation_is_a_different_yardstick(weights, pair, f64, ref_dev):
    dev = (R.raft_forward(raft.fold_batchnorm(weights), *pair, UPDATES, torch.float64, rnd=R.fp16_round) - f64).abs().max().item()
    print(f"fp16 emulation deviation {dev:.3e} px")
    assert 4 * ref_dev < dev < 1.0


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_comparison_rejects_defect(weights, pair, f64, ref_dev, defect):
    err = (R.raft_forward(weights, *pair, UPDATES, torch.float64, defect=defect) - f64).abs().max().item()
    print(f"{defect}: {err:.3e} px against 4 x ref_dev = {4 * ref_dev:.3e}")
    assert err > 100 * 4 * ref_dev


def test_minimum_feature_map(weights):
    x = torch.zeros(1, 3, 120, 136)
    with pytest.raises(ValueError, match="16 x 16"):
        R.raft_forward(weights, x, x, 1)


def test_return_at_matches_separate_runs(weights, pair):
    many = R.raft_forward(weights, *pair, 3, torch.float64, return_at=(1, 3))
    assert torch.equal(many[1], R.raft_forward(weights, *pair, 1, torch.float64))
    assert torch.equal(many[3], R.raft_forward(weights, *pair, 3, torch.float64))


# ---- loader strictness and the weight naming
def test_weight_naming(weights):
    raft.check_state_dict(weights)
    for key in ("feature_encoder.convnormrelu.0.weight", "feature_encoder.layer2.0.downsample.0.bias", "feature_encoder.conv.weight",
                "context_encoder.layer3.1.convnormrelu2.1.running_var", "context_encoder.convnormrelu.1.num_batches_tracked",
                "update_block.motion_encoder.convcorr1.0.weight", "update_block.motion_encoder.convflow1.0.weight",
                "update_block.motion_encoder.conv.0.bias", "update_block.recurrent_block.convgru1.convz.weight",
                "update_block.recurrent_block.convgru2.convq.bias", "update_block.flow_head.conv2.weight",
                "mask_predictor.convrelu.0.weight", "mask_predictor.conv.bias"):
        assert key in weights, key
    assert weights["update_block.recurrent_block.convgru1.convz.weight"].shape == (128, 384, 1, 5)
    assert weights["update_block.recurrent_block.convgru2.convz.weight"].shape == (128, 384, 5, 1)
    assert weights["update_block.motion_encoder.conv.0.weight"].shape == (126, 256, 3, 3)
    assert weights["mask_predictor.conv.weight"].shape == (576, 256, 1, 1)
    assert not any(k.startswith("feature_encoder") and "running" in k for k in weights)     # instance norm: no parameters
    assert sorted(s.index for s in raft.raft_large_convs()) == list(range(32)) + list(range(33, 48))   # 32: the context half of 31
    again = synth.make_raft_weights(0)
    assert all(torch.equal(weights[k], again[k]) for k in weights)
    other = synth.make_raft_weights(1)
    assert not torch.equal(weights["feature_encoder.conv.weight"], other["feature_encoder.conv.weight"])
    # the two scaled convolutions: Kaiming fan-out std sqrt(2 / fan_out) times 0.01 / 0.1
    assert abs(weights["update_block.flow_head.conv2.weight"].std().item() / (0.01 * (2 / 18) ** 0.5) - 1) < 0.1
    assert abs(weights["feature_encoder.conv.weight"].std().item() / (0.1 * (2 / 256) ** 0.5) - 1) < 0.1
    assert abs(weights["update_block.flow_head.conv1.weight"].std().item() / (2 / (256 * 9)) ** 0.5 - 1) < 0.1


def test_loader_is_strict(weights):
    sd = dict(weights)
    del sd["update_block.flow_head.conv1.bias"]
    with pytest.raises(KeyError, match="update_block.flow_head.conv1.bias"):
        raft.check_state_dict(sd)
    sd = dict(weights, **{"feature_encoder.extra.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match="feature_encoder.extra.weight"):
        raft.check_state_dict(sd)
    sd = dict(weights)
    sd["mask_predictor.conv.weight"] = torch.zeros(576, 256, 3, 3)
    with pytest.raises(ValueError, match="mask_predictor.conv.weight"):
        raft.check_state_dict(sd)
    with pytest.raises(ValueError, match="operands"):
        raft.RaftLarge(weights, "cuda:0", operands="bf16")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.RaftLarge(weights, "cpu")


def test_weight_scale_is_a_power_of_two():
    for m in (1e-4, 0.03, 0.9, 1.0, 37.0):
        s = raft.weight_scale(torch.tensor([m, -m / 3]))
        assert 128 <= m * s < 256 and s == 2.0 ** round(torch.log2(torch.tensor(s)).item())
    assert raft.weight_scale(torch.zeros(3)) == 1.0


def test_pad_to_8():
    assert raft.pad_to_8(131, 141) == [1, 2, 2, 3] and raft.pad_to_8(128, 136) == [0, 0, 0, 0] and raft.pad_to_8(476, 854) == [1, 1, 2, 2]


def test_ctypes_mirrors_match_header():
    """dtk_raft_conv_desc / dtk_raft_conv_args / dtk_raft_model: the header's fields in the header's order, the implied sizes, and
    the DTK_RAFT_* constants the Python side repeats."""
    import ctypes
    import os
    import re
    from dino_tracker_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dtk.h")).read()

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        decls = re.findall(r"(?:const void\*|const float\*|float\*|int64_t|int32_t|float|dtk_raft_conv_desc)\s+([^;]+);", body)
        return [re.sub(r"\[.*", "", f.strip()) for d in decls for f in d.split(",")]

    assert fields("dtk_raft_conv_desc") == [n for n, _ in _lib.RaftConvDesc._fields_]
    assert [f if f != "in" else "in_" for f in fields("dtk_raft_conv_args")] == [n for n, _ in _lib.RaftConvArgs._fields_]
    assert fields("dtk_raft_model") == ["conv"]
    assert ctypes.sizeof(_lib.RaftConvDesc) == 3 * 8 + 7 * 4 + 4
    assert ctypes.sizeof(_lib.RaftConvArgs) == 56 + 8 * 4 + 6 * 8 + 6 * 8
    for name, value in (("NUM_CONVS", _lib.RAFT_NUM_CONVS), ("SPLIT", _lib.RAFT_SPLIT), ("FP16", _lib.RAFT_FP16),
                        ("ACT_NONE", _lib.RAFT_ACT_NONE), ("ACT_RELU", _lib.RAFT_ACT_RELU), ("ACT_SIGMOID", _lib.RAFT_ACT_SIGMOID),
                        ("ACT_TANH", _lib.RAFT_ACT_TANH), ("CONTEXT_HIDDEN", 31), ("CONTEXT_CONTEXT", 32), ("MOTION", 33), ("GRU", 38),
                        ("FLOW_HEAD", 44), ("MASK", 46)):
        assert int(re.search(r"#define DTK_RAFT_%s (\d+)" % name, text).group(1)) == value, name
    assert ctypes.sizeof(_lib.RaftModel) == _lib.RAFT_NUM_CONVS * ctypes.sizeof(_lib.RaftConvDesc)
    index = {s.key: s.index for s in raft.raft_large_convs()}
    assert index["update_block.motion_encoder.convcorr1.0"] == 33 and index["update_block.recurrent_block.convgru1.convz"] == 38
    assert index["update_block.flow_head.conv1"] == 44 and index["mask_predictor.convrelu.0"] == 46
    assert index["context_encoder.convnormrelu.0"] == 16 and index["context_encoder.conv"] == 31
