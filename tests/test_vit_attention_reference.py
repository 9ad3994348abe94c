"""CPU: the test of tests/vit_attention_ref.py, the helper tests/test_gpu_vit_attention_shapes.py holds the attention kernels to.

  * `reference` is scaled-dot-product attention: it agrees with torch's own in float64 once the exp2-domain scaling is undone;
  * the crafted rows of every shape of the table are what the builder says they are, for the committed seeds, in fp32 and after
    rounding to either operand type (a row that is not extreme forces no branch of the kernels' guard logic);
  * the reference does not read the padding: zero and finite padding give bit-identical references."""
import pytest
import torch

import vit_attention_ref as R

IDS = [R.shape_id(s) for s in R.SHAPES]


@pytest.mark.parametrize("shape", [R.SHAPES[3], R.SHAPES[6]], ids=[IDS[3], IDS[6]])
def test_reference_is_scaled_dot_product_attention(shape):
    S, Sp, F, H, seed = shape
    q, k, v, _ = R.make_case(S, Sp, F, H, seed, "finite")
    ref = R.reference(q, k, v, S)
    assert ref.dtype == torch.float64 and ref.shape == (F, S, H * 64)
    qd, kd, vd = q.double()[:, :, :S] / R.QS, k.double()[:, :, :S], v.double()[:, :, :S]     # back to plain q: scale 1 / sqrt(64)
    sdpa = torch.nn.functional.scaled_dot_product_attention(qd, kd, vd).permute(0, 2, 1, 3).reshape(F, S, H * 64)
    assert (ref - sdpa).abs().max().item() < 1e-12
    assert R.row_rel(ref, ref).shape == (F, S) and R.row_rel(ref, ref).max() == 0
    # the metric: one output of one row moved by 1 % of the row's largest value reads 0.01 in that row and 0 elsewhere
    f, r = F - 1, S // 2
    moved = ref.clone()
    moved[f, r, 5] += 0.01 * max(ref[f, r].abs().max().item(), 0.05)
    rel = R.row_rel(moved, ref)
    assert abs(rel[f, r].item() - 0.01) < 1e-12 and rel.sum().item() == rel[f, r].item()


@pytest.mark.parametrize("pads", ["zero", "finite"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_crafted_rows_are_what_the_builder_claims(shape, pads):
    S, Sp, F, H, seed = shape
    q, k, v, crafted = R.make_case(S, Sp, F, H, seed, pads)
    ntiles = (S + 63) // 64
    for x in (q, k, v):
        assert x.shape == (F, H, Sp, 64) and x.dtype == torch.float32 and torch.isfinite(x).all()
        if pads == "zero":
            assert not x[:, :, S:].any()
        elif Sp > S:
            assert x[:, :, S:].abs().max() <= 3 and x[:, :, S:].abs().max() > 2 and (x[:, :, S:] != 0).all()
    tags = [c[3] for c in crafted]
    assert tags.count("all-negative") == len({0, S - 1} | ({S - 33} if S > 32 else set()))
    assert tags.count("sharp") == 1 and tags.count("late-tile") == (1 if ntiles >= 2 else 0)
    assert all(0 <= f < F and 0 <= h < H and 0 <= r < S for f, h, r, _ in crafted)
    assert R.tag_of(crafted, F - 1, H - 1, S - 1).endswith("sharp")
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        for tag, where, ok, fig in R.crafted_row_claims(q.to(dt), k.to(dt), S, crafted):
            assert ok, (tag, where, fig, dt)


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_reference_does_not_read_the_padding(shape):
    S, Sp, F, H, seed = shape
    qz, kz, vz, cz = R.make_case(S, Sp, F, H, seed, "zero")
    qf, kf, vf, cf = R.make_case(S, Sp, F, H, seed, "finite")
    assert cz == cf
    if Sp > S:
        assert not torch.equal(qz, qf) and not torch.equal(kz, kf) and not torch.equal(vz, vf)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        assert torch.equal(R.reference(qz.to(dt), kz.to(dt), vz.to(dt), S), R.reference(qf.to(dt), kf.to(dt), vf.to(dt), S))


def test_raised_bounds_are_exactly_the_cases_the_format_alone_exceeds():
    """EMULATED_BEYOND_TOL lists (type, S) -> the row-relative error of the float64 emulation that rounds only P and the output to the
    type.  It must hold exactly the cases of the table in which that emulation exceeds the bound of dtk_vit_attention, with the
    emulated figure: no case gets a wider bound for any other reason, and the figure is not taken from a kernel.  Against the row
    maximum instead of the kernels' estimated reference the same emulation stays inside the bound: the excess is where P falls on the
    mantissa grid, not a larger class of error."""
    beyond = {}
    for dtn, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        for S, Sp, F, H, seed in R.SHAPES:
            q, k, v, _ = R.make_case(S, Sp, F, H, seed, "zero")
            qb, kb, vb = q.to(dt), k.to(dt), v.to(dt)
            ref = R.reference(qb, kb, vb, S)
            e = R.row_rel(R.emulated_16bit(qb, kb, vb, S, dt), ref).max().item()
            assert e == e and R.row_rel(R.emulated_16bit(qb, kb, vb, S, dt, "max"), ref).max().item() < R.TOL["fast", dtn]
            if e >= R.TOL["fast", dtn]:
                beyond[dtn, S] = e
            assert R.fast_bound(dtn, S) == (2 * R.EMULATED_BEYOND_TOL[dtn, S] if (dtn, S) in beyond else R.TOL["fast", dtn])
            assert R.fast_bound(dtn, S) < 2.5 * R.TOL["fast", dtn]
    assert sorted(beyond) == sorted(R.EMULATED_BEYOND_TOL)
    for key, e in beyond.items():
        assert abs(e - R.EMULATED_BEYOND_TOL[key]) < 1e-3 * e, (key, e)
