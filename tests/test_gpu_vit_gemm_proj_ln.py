"""-m gpu: the attention projection of ViT-S with LayerNorm-2 in its epilogue (csrc/vit_gemm_ws_ln.h: gemm_ws_ln_kernel, role PROJ with
ln_out at D = 384) -- the stage alone against float64 and against the two-launch form, the encoder with and without the fusion, the
fp16 range word and the refusals.  Operands, references and bounds are those of tests/vit_gemm_ref.py; the stage is driven by
tests/test_gpu_vit_gemm.py's run_stage (guard bands behind every output, `out` must come back untouched).

Row counts come from the kernel's grid: a chunk of consecutive 32-row tiles per workgroup, G = the device's CU count workgroups at most
(gemm_ws_ln_grid).  1 / 31 / 32 / 33 / 95 rows: fewer tiles than workgroups, M < 32, partial last tiles of 1 and 31 rows;
32 G - 1: one tile per workgroup; 32 G + 17 and 64 G + 17: two and three tiles per workgroup (32 G + 17: a last chunk of one tile) and a
last tile of 17 rows."""
import pytest
import torch

import vit_gemm_ref as R
from dino_tracker_amd import _lib, synth
from dino_tracker_amd.extractor import VitExtractor
from test_gpu_vit_gemm import BF16, DEV, F16, run_stage

pytestmark = pytest.mark.gpu

D = 384


def _G():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _row_counts():
    G = _G()
    rows = [1, 31, 32, 33, 95, 32 * G - 1, 32 * G + 17, 32 * (2 * G) + 17]
    # tiles per chunk as gemm_ws_ln_grid computes them: 1, 2 and 3 tiles per workgroup
    for r, tpc_want in zip(rows[-3:], (1, 2, 3)):
        tiles = -(-r // 32)
        tpc = -(-tiles // G)
        assert tpc == tpc_want, (r, tiles, tpc)
    return rows


def _ln_bound(o, x, ref, n):
    """|ln_out - LayerNorm64(x)| allowed in the realistic class: half an ulp of T for the final rounding; the fp32 mean of 384 terms
    in any order is off by at most 384 u mean|x|, which moves n by that times rstd; the variance sum likewise moves rstd by a relative
    384 u (half of the variance's 2 x 384 u) plus a few roundings; the expression (x - mean) * rstd * w + b adds ~4 roundings of
    |n w| + |b|.  C_ACC = 2 as for the GEMM sums."""
    x = x.double()
    mu = x.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(dim=1, keepdim=True) + o["ln_eps"])
    w, b = o["ln_w"].double().abs(), o["ln_b"].double().abs()
    dn = R.C_ACC * D * R.U32 * (x.abs().mean(dim=1, keepdim=True) * rstd + n.abs()) + 4 * R.U32 * n.abs()
    return 0.5 * R.ulp(ref, o["dtype"]) + dn * w + 4 * R.U32 * (n.abs() * w + b)


@pytest.mark.parametrize("cls", ["exact", "real"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_proj_ln_stage_vs_float64(dt, cls):
    """Role PROJ with ln_out at every row count of the module docstring.  Exact class: x bit-equal to fp32(x_in + T(exact update)),
    ln_out within one ulp of the float64 LayerNorm of it.  Realistic class: x within the derived bound of tests/vit_gemm_ref.py,
    ln_out within _ln_bound of the float64 LayerNorm of the x the kernel wrote.  Guard bands and `out`: run_stage."""
    dtype = F16 if dt == "fp16" else BF16
    worst = (0.0, None, None)
    worst_ln = 0.0
    for i, rows in enumerate(_row_counts()):
        seed = 4241 + 13 * i + (dt == "bf16")
        if cls == "exact":
            o = R.make_exact(R.PROJ, D, rows, dtype, seed, device=DEV, fused_ln=True)
            R.check_exact(o, run_stage(o, 0, fused=True))
        else:
            o = R.make_real(R.PROJ, D, rows, dtype, seed, device=DEV, fused_ln=True)
            got = run_stage(o, 0, fused=True)
            ratio, at = R.check_real(o, got)
            if ratio > worst[0]:
                worst = (ratio, rows, at)
            ref, n = R.layernorm64(got["x"], o["ln_w"], o["ln_b"], o["ln_eps"])
            r_ln = ((got["ln_out"].double() - ref).abs() / _ln_bound(o, got["x"], ref, n)).max().item()
            worst_ln = max(worst_ln, r_ln)
            assert r_ln <= 1.0, (rows, r_ln)
    if cls == "exact":
        print(f"vit_gemm proj+ln {dt} exact: {len(_row_counts())} row counts, x bit-equal, ln_out within one ulp")
    else:
        print(f"vit_gemm proj+ln {dt} real: worst |x - ref| / bound = {worst[0]:.3f} at rows={worst[1]} (row, col)={worst[2]}; "
              f"worst |ln_out - ref| / bound = {worst_ln:.3f}")


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_proj_ln_matches_two_launch_form(dt):
    """The same operands through the unfused projection of the same library give the 16-bit update `delta`; the fused stage's x must
    equal x_in + float(delta) bit for bit (realistic operands: every rounding of the update counts)."""
    dtype = F16 if dt == "fp16" else BF16
    G = _G()
    for i, rows in enumerate((95, 32 * G + 17)):
        o = R.make_real(R.PROJ, D, rows, dtype, 977 + i, device=DEV, fused_ln=True)
        got = run_stage(o, 0, fused=True)
        o2 = {k: v for k, v in o.items() if k not in ("x", "ln_w", "ln_b", "ln_eps")}
        delta = run_stage(o2, 0)["out"]
        bad = got["x"] != o["x"] + delta.float()
        assert not bad.any(), (rows, int(bad.sum()))


def test_encoder_with_and_without_the_fusion_is_bit_identical():
    """ViT-S on three frames of 154 x 238 (S = 694: rows % 32 != 0, tiles crossing frame ends) and of 140 x 154, layer 2 and the default
    layer: the default encoder (five launches per block) against no_ln_fusion (both LayerNorms as launches of their own), features
    and tokens."""
    name = "dinov2_vits14"
    sd = synth.make_vit_weights(name, seed=9, layerscale=0.1)
    for hw in ((154, 238), (140, 154)):
        video = synth.synth_video(3, hw[0], hw[1], seed=84)
        for layer in (2, None):
            out = {}
            for form in ("new", "unfused"):
                ex = VitExtractor(name, stride=7, device="cuda:0", state_dict=sd)
                ex.no_ln_fusion = form == "unfused"
                out[form] = (ex.encode(video, layer=layer), ex.encode(video, layer=layer, want="tokens"))
            assert torch.isfinite(out["new"][0]).all()
            assert torch.equal(out["new"][0], out["unfused"][0]), (hw, layer, "features")
            assert torch.equal(out["new"][1], out["unfused"][1]), (hw, layer, "tokens")


def test_proj_ln_range_word():
    """The recipe of test_overflow_word for the residual update: ONE product sum of 65536 (256 products of 16 x 16, LayerScale 1) in the
    last valid row saturates the fp16 update -- bit 0 of the word, and x (zero before) receives 65504; with 255 products (65280) the
    word stays 0; bf16 operands never touch the word."""
    rows, N = 3 * 32 + 17, D

    def craft(dtype, terms):
        A, W = torch.zeros(rows, D, device=DEV), torch.zeros(N, D, device=DEV)
        A[rows - 1, :terms] = 16.0
        W[N - 1, :256] = 16.0
        return {"role": R.PROJ, "D": D, "rows": rows, "dtype": dtype, "split": False, "w_scale": 1.0, "exact": False,
                "A": A.to(dtype), "W": W.to(dtype), "bias": torch.zeros(N, device=DEV), "gamma": torch.ones(N, device=DEV),
                "x": torch.zeros(rows, N, device=DEV), "ln_w": torch.ones(N, device=DEV), "ln_b": torch.zeros(N, device=DEV), "ln_eps": 1e-6}

    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    for dtype, terms, word0, want_word, want_x in ((F16, 256, 0, 1, 65504.0), (F16, 255, 0, 0, 65280.0), (BF16, 256, 0x40, 0x40, 65536.0)):
        word.fill_(word0)
        got = run_stage(craft(dtype, terms), 0, fused=True, ovf=word)
        x = got["x"]
        assert int(word) == want_word and float(x[rows - 1, N - 1]) == want_x, (dtype, terms, int(word), float(x[rows - 1, N - 1]))
        x[rows - 1, N - 1] = 0.0
        assert not x.any(), "an update outside the crafted element"


@pytest.mark.parametrize("flags", [_lib.VIT_TILED_GEMMS, _lib.VIT_NO_LN_FUSION], ids=["tiled_gemms", "no_ln_fusion"])
def test_proj_ln_is_refused_where_the_encoder_does_not_fuse(flags):
    o = R.make_exact(R.PROJ, D, 64, F16, 1, device=DEV, fused_ln=True)
    with pytest.raises(RuntimeError, match="fused LayerNorm"):
        run_stage(o, flags, fused=True)
