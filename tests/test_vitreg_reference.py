"""CPU: the reference that the register-model GPU tests are judged by (tests/vitreg_ref.py) is itself checked, and so are the parts of the
feature that need no GPU --
(1) with R = 0 the restatement is the oracle's encoder, (2) with registers it is transformers' Dinov2WithRegistersModel, (3) the cases of
the GPU tests are sensitive to their registers by 10 x the tolerance that guards them, (4) the comparison the GPU tests use accepts a
float32 run of the restatement and rejects five planted defects, (5) synth / VitExtractor's static facts / the ABI mirror / the overlay."""
import ctypes
import hashlib
import os
import subprocess
import sys

import pytest
import torch

import vitreg_ref as V
from dino_tracker_amd import _lib, synth
from oracle import ref_algo as A

REG_NAMES = ["dinov2_vits14_reg", "dinov2_vitb14_reg", "dinov2_vitl14_reg", "dinov2_vitg14_reg"]


# ---- (1) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [7, 14])
def test_without_registers_it_is_the_oracle(stride):
    """float64 restatement against the float32 oracle (oracle.ref_algo.vit_all_tokens) on the plain ViT-S weights: tokens and the qkv record
    of block 1.  The bound is the float32 oracle's own rounding: tests/vitg_ref.py / the oracle agree to ~1e-6 relative (measured here:
    5e-7, the figure of every float32 run of these two blocks in docs/PARITY.md); 2e-6 leaves a factor 4 and is 4 orders below a row out of
    place."""
    sd = synth.make_vit_weights("dinov2_vits14", seed=V.SEED_WEIGHTS, nblocks=2)
    video = synth.synth_video(2, 98, 126, seed=V.SEED_VIDEO)
    with torch.no_grad():
        tok32, qkv32 = A.vit_all_tokens(video, sd, "dinov2_vits14", layer=1, stride=stride, return_qkv=True)
        got = V.encode(video.double(), V.to64(sd), 1, heads=6, stride=stride)
    assert V.n_registers(sd) == 0 and got["tokens"].shape == tok32.shape
    rt, rq = V.rel(tok32, got["tokens"]), V.rel(qkv32, got["qkv"])
    print(f"vitreg_ref with R = 0 vs the float32 oracle, stride {stride}: tokens rel {rt:.2e}, qkv rel {rq:.2e}")
    assert rt <= 2e-6 and rq <= 2e-6
    assert torch.equal(got["feat"], got["tokens"][:, 1:])


# ---- (2) ------------------------------------------------------------------------------------------------------------------------------
def test_matches_transformers_dinov2_with_registers():
    """tests/hf_registers_crosscheck.py in a clean interpreter (as test_vitg_reference.py runs its cross-check: the torchvision shim that
    other tests install for the reference must not be visible to transformers)."""
    pytest.importorskip("transformers")
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hf_registers_crosscheck.py")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr


# ---- (3) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(V.CASES))
def test_gpu_cases_are_sensitive_to_their_registers(key):
    """A device that ignored its registers (or got them wrong) must not pass: for the weights and frames of every GPU case, the float64
    patch features of the tested block with and without registers differ by >= 10 x the tolerance of the comparison that guards them -- the
    fast-fp16 class (8e-4), which also covers the tighter split comparison.  The bf16 class (2e-2) is wider than the whole effect of four
    tokens among 226, so the bf16 comparison of the main case does not guard the registers; the one-patch case, where four of six tokens are
    registers, is run on bf16 too and is held to 10 x that class here."""
    s = V.register_sensitivity(key)
    print(f"register sensitivity of case {key} {V.CASES[key]}: {s:.3e} (register scale {synth.REGISTER_STD})")
    assert s >= 10 * V.FP16_TOL["rel_max"]
    if key == "one":
        assert s >= 10 * V.BF16_TOL["rel_max"]


# ---- (4) ------------------------------------------------------------------------------------------------------------------------------
def test_comparison_accepts_float32_and_rejects_planted_defects():
    c = V.make_case("main")
    ref, ref32 = c["ref"][c["layer"]], c["ref32"]
    fig = V.check_records(ref32, ref, **V.FP16_TOL)
    print("float32 restatement vs float64, main case:", {k: f"{v[1]:.2e}" for k, v in fig.items()})
    for k in ("tokens", "feat", "qkv"):
        V.check_split(ref32[k], ref[k], ref32[k])
    plain = V.encode(c["video"], V.without_registers(c["sd"]), -1, c["heads"])["tokens"]
    V.check_embedding_exact(V.encode(c["video"], c["sd"], -1, c["heads"])["tokens"], plain, c["sd"]["register_tokens"])
    for d in V.DEFECTS:
        with torch.no_grad():
            bad = V.encode(c["video"], c["sd"], c["layer"], c["heads"], defect=d)
        with pytest.raises(AssertionError):
            V.check_records(bad, ref, **V.FP16_TOL)
        # the split comparison on its own, and the exact comparison where the defect is in the embedding
        with pytest.raises(AssertionError):
            for k in ("tokens", "feat", "qkv"):
                V.check_split(bad[k], ref[k], ref32[k])
        if d in ("reg_pos", "reg_after", "reg_zero"):
            with pytest.raises(AssertionError):
                V.check_embedding_exact(V.encode(c["video"], c["sd"], -1, c["heads"], defect=d)["tokens"], plain, c["sd"]["register_tokens"])
    # a device that ignored the registers altogether, judged on the features alone
    with torch.no_grad():
        ignored = V.encode(c["video"], V.without_registers(c["sd"]), c["layer"], c["heads"])
    with pytest.raises(AssertionError):
        V.check(ignored["feat"], ref["feat"], **V.FP16_TOL)


# ---- (5) ------------------------------------------------------------------------------------------------------------------------------
def test_configs_and_synthetic_weights():
    for name in REG_NAMES:
        plain = name[:-4]
        assert synth.VIT_CONFIGS[name] == dict(synth.VIT_CONFIGS[plain], registers=4)
        assert "registers" not in synth.VIT_CONFIGS[plain]
    for name in ("dinov2_vits14_reg", "dinov2_vitg14_reg"):
        sd, sib = synth.make_vit_weights(name, seed=5, nblocks=1), synth.make_vit_weights(name[:-4], seed=5, nblocks=1)
        d = synth.VIT_CONFIGS[name]["dim"]
        assert sd["register_tokens"].shape == (1, 4, d) and "register_tokens" not in sib
        assert set(sd) == set(sib) | {"register_tokens"} and all(torch.equal(sd[k], sib[k]) for k in sib)
        assert sd["pos_embed"].shape == (1, 1 + 37 * 37, d)
    # the scale: comparable to a patch token's norm
    c = V.make_case("main")
    tok = c["ref"][c["layer"]]["tokens"]
    e = V.embed(c["video"], c["sd"])
    ratio = float(e[:, 1:5].norm(dim=-1).mean() / e[:, 5:].norm(dim=-1).mean())
    print(f"synthetic register norm / patch-token norm at the embedding: {ratio:.2f}")
    assert 0.5 <= ratio <= 2.0 and tok.shape == (3, 226, 384)


PARENT_HASHES = {   # sha256 over sorted(name, tensor bytes) of make_vit_weights(name, seed=2) (tests/test_vitg_reference.py records the first three)
    "dinov2_vits14": "b8666e34730bbd7bd59ae50bc929a73aa9a621164ad077e6b3d3cd10175484d9",
}


def test_plain_weights_unchanged():
    sd = synth.make_vit_weights("dinov2_vits14", seed=2)
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    assert h.hexdigest() == PARENT_HASHES["dinov2_vits14"]


def test_static_facts_come_from_the_config_not_from_letters():
    """"g" is in "reg": the layer count, head count and width of a _reg name must be its sibling's (VIT_CONFIGS is the source of truth)."""
    from dino_tracker_amd.extractor import VitExtractor
    for name in REG_NAMES:
        cfg = synth.VIT_CONFIGS[name[:-4]]
        ex = VitExtractor.__new__(VitExtractor)            # the static facts only: no device, no weights
        torch.nn.Module.__init__(ex)
        ex.model_name, ex.stride, ex.cfg, ex.n_registers = name, 7, synth.VIT_CONFIGS[name], synth.VIT_CONFIGS[name]["registers"]
        assert ex.get_n_layers() == cfg["depth"] and ex.get_head_num() == cfg["heads"]
        assert VitExtractor.get_embedding_dim(name) == cfg["dim"] and ex.get_patch_size() == 14
        shape = (1, 3, 98, 126)
        assert (ex.get_height_patch_num(shape), ex.get_width_patch_num(shape)) == (13, 17)
        assert ex.get_patch_num(shape) == 1 + 4 + 13 * 17
    with pytest.raises(NotImplementedError):
        VitExtractor("dinov2_vits14_reg4", stride=7, device="cpu", random_seed=1)


def test_state_dict_and_name_must_agree():
    """Checked before anything touches a device: a plain name with register_tokens, a _reg name without them or with the wrong shape."""
    from dino_tracker_amd.extractor import VitExtractor
    reg = synth.make_vit_weights("dinov2_vits14_reg", seed=5, nblocks=1)
    with pytest.raises(ValueError, match="register_tokens"):
        VitExtractor("dinov2_vits14", stride=7, device="cpu", state_dict=reg)
    with pytest.raises(KeyError, match="register_tokens"):
        VitExtractor("dinov2_vits14_reg", stride=7, device="cpu", state_dict=V.without_registers(reg))
    bad = dict(reg, register_tokens=reg["register_tokens"][:, :3])
    with pytest.raises(ValueError, match="register_tokens"):
        VitExtractor("dinov2_vits14_reg", stride=7, device="cpu", state_dict=bad)


def test_vit_model_mirror_has_the_register_fields():
    names = [f[0] for f in _lib.VitModel._fields_]
    assert names[-4:] == ["ffn", "hidden", "n_registers", "registers"]
    m = _lib.VitModel(384, 6)                        # trailing fields default to zero: today's model
    assert m.n_registers == 0 and not m.registers
    assert _lib.VitModel.n_registers.size == 4 and _lib.VitModel.registers.size == ctypes.sizeof(ctypes.c_void_p)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dtk.h")).read()
    body = header[header.index("typedef struct dtk_vit_model {"):header.index("} dtk_vit_model;")]
    assert body.index("int32_t hidden;") < body.index("int32_t n_registers;") < body.index("const float* registers;")


def test_overlay_passes_the_model_name_through():
    """A `dino_model_name: dinov2_vitl14_reg` of a preprocessing config reaches VitExtractor: the reference's save_dino_embed_video.py calls
    utils.get_dino_features_video(model_name=config["dino_model_name"], ...), the overlay's utils re-exports the package's function, and
    that function hands the name to VitExtractor unchanged (seen here as the extractor's own complaint about the missing weights)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("overlay_utils_for_vitreg", os.path.join(root, "overlay", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from dino_tracker_amd import utils
    assert mod.get_dino_features_video is utils.get_dino_features_video
    config = {"dino_model_name": "dinov2_vitl14_reg", "dino_stride": 7, "dino_layer": 23, "dino_facet": "tokens"}
    sd = V.without_registers(synth.make_vit_weights("dinov2_vitl14_reg", seed=5, nblocks=1))
    with pytest.raises(KeyError, match="dinov2_vitl14_reg.*register_tokens"):
        mod.get_dino_features_video(video=torch.zeros(1, 3, 28, 28), model_name=config["dino_model_name"], facet=config["dino_facet"],
                                    stride=config["dino_stride"], layer=config["dino_layer"], device="cpu", state_dict=sd)
