"""-m gpu: the three ViT attention kernels on their own -- attention6_kernel (csrc/vit_attention6.h, the default), attention4_kernel
(csrc/vit_attention4.h, DTK_OPERAND_ATTENTION_V4) through dtk_vit_attention, attention_split_kernel (csrc/vit_split.h) through
dtk_vit_attention_split -- at the token counts at which their control flow changes, against float64 on the operands they were given
(tests/vit_attention_ref.py; the builder's claims are checked on the CPU by tests/test_vit_attention_reference.py).

What a shape of the table (vit_attention_ref.SHAPES) pins, ntiles = ceil(S / 64):
  S % 64 == 0           no masked tail: attention6's tail_tile = -1, neither mask_tail site of attention4's loop, the split kernel's
                        (kt + 1) * AS_KEYS > S test not taken (64, 128, 320, 384); Sp == S
  ntiles = 1, 2, 3      the prologue of both fast kernels requests tiles 0 .. 2 as min(t, ntiles - 1); attention4's `ntiles == 1` mask
                        (33) and its `t + 1 == ntiles - 1` mask on an odd position (65: a one-key tail); attention6's first key tile
  ntiles % 4 = 1, 2, 3  the unrolled ring tails `if (t + k < ntiles)` (257 and 320: 5, 384: 6, 577: 10, 129: 3; 222 and 705: 0)
  queries beyond S      a wave or a workgroup with one valid row or none: Q rows clamped to Sp - 1, the estimate's own 32 keys all
                        masked, no store (33: the second 32-query tile; 129: the split kernel's second workgroup; 257: attention4's;
                        513: attention6's, whose waves 1 .. 3 hold nothing)
  Sp - S >= 64          a whole padding tile beyond ntiles (129)
  F H > 8               fh = (seq / QB) * 8 + xcd, qb = seq % QB beyond the first eight pairs, with QB = 2 (513: 3 x 3) and with idle
                        workgroups that return early (F H = 9, 10, 12)
  crafted rows          a guard pending when the key loop ends (late-tile), a safe pass in the wave that straddles S (sharp), rows whose
                        every score is far below 0 (all-negative: one unmasked zero key would take their whole softmax)
  pads = "finite"       include/dtk.h promises that the padding rows of K and the padding columns of V^T only have to be finite

Every output is written into the middle of a larger buffer whose margins must come back untouched.  Bounds: those of the two existing
stand-alone tests for the same metric (16-bit P and 16-bit output: 2^-11 fp16, 2^-8 bf16; the split stage's fp32-grade figures).  The
zero-pad and finite-pad runs are NOT compared with each other: a finite padding Q row may send its wave through the safe pass, which
rounds the wave's valid rows differently; both are held to float64."""
import functools

import pytest
import torch

import vit_attention_ref as R
from dino_tracker_amd import ops
from dino_tracker_amd._lib import OPERAND_ATTENTION_V4, OPERAND_BF16, OPERAND_F16, check, lib

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC1          # a NaN in both 16-bit types: an output element nobody wrote fails the finiteness check


def _split(x, dt):
    hi = x.to(dt)
    lo = (x - hi.float()).to(dt)
    return hi, lo


@functools.lru_cache(maxsize=None)
def _host_case(shape, dt, split, pads):
    """Host operands in the layouts of the entry point, the float64 reference on them and the crafted rows; built once per
    (shape, type, fast / split, pads) and shared by the kernels that read the same operands."""
    S, Sp, F, H, seed = shape
    tdt = torch.float16 if dt == "fp16" else torch.bfloat16
    q, k, v, crafted = R.make_case(S, Sp, F, H, seed, pads)
    if split:
        planes = []
        for x, tr in ((q, False), (k, False), (v, True)):
            hi, lo = _split(x.transpose(2, 3).contiguous() if tr else x, tdt)
            planes += [hi.contiguous(), lo.contiguous()]
        seen = [planes[2 * i].double() + planes[2 * i + 1].double() for i in range(3)]     # what the device sees: hi + lo
        ref = R.reference(seen[0], seen[1], seen[2].transpose(2, 3), S)
    else:
        qb, kb, vb = q.to(tdt), k.to(tdt), v.to(tdt)
        planes = [qb.contiguous(), kb.contiguous(), vb.transpose(2, 3).contiguous()]       # V^T: [F][H][64][Sp]
        ref = R.reference(qb, kb, vb, S)
    for i, p in enumerate(planes):   # exactly the documented sizes: q, k [F][H][Sp][64], then V^T [F][H][64][Sp]
        assert p.shape == ((F, H, 64, Sp) if i * 3 // len(planes) == 2 else (F, H, Sp, 64)) and p.dtype == tdt
    return planes, ref, crafted


def _guarded(n, guard, tdt):
    buf = torch.full((guard + n + guard,), SENTINEL, dtype=torch.int16, device="cuda")
    return buf, buf[guard:guard + n].view(tdt)


@pytest.mark.parametrize("pads", ["zero", "finite"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=[R.shape_id(s) for s in R.SHAPES])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("kernel", ["v6", "v4", "split"])
def test_attention_at_small_and_boundary_token_counts(kernel, dt, shape, pads):
    """Bounds on the largest row-relative error: dtk_vit_attention 1e-3 (fp16) / 6e-3 (bf16), the split stage 2e-5 / 4e-3 -- except
    four bf16 cases of dtk_vit_attention in which the rounding of P and of the output to bf16, emulated in float64 from the operands
    (vit_attention_ref.emulated_16bit: nothing else is rounded), is by itself beyond 6e-3: S = 222: 6.655e-3, S = 320: 6.084e-3,
    S = 384: 7.090e-3, S = 577: 7.141e-3, each on a plain row.  Those cases are held to twice the emulated figure.  (Measured on an
    MI355X: with bf16 operands both fast kernels, under both paddings, land on the emulated figure to three digits at EVERY shape of
    the table, these four included -- they round P and the output and nothing else; fp16 stays below 1e-3 everywhere, at most 9.2e-4
    at S = 577.)"""
    S, Sp, F, H, _ = shape
    split = kernel == "split"
    tdt = torch.float16 if dt == "fp16" else torch.bfloat16
    ot = OPERAND_F16 if dt == "fp16" else OPERAND_BF16
    planes, ref, crafted = _host_case(shape, dt, split, pads)
    dev = [p.cuda() for p in planes]
    n, guard = F * S * H * 64, 64 * H * 64
    bufs, outs = zip(*[_guarded(n, guard, tdt) for _ in range(2 if split else 1)])
    outs = [o.view(F, S, H * 64) for o in outs]
    if split:
        check(lib().dtk_vit_attention_split(*[ops._p(t) for t in dev], ops._p(outs[0]), ops._p(outs[1]), F, H, S, Sp, ot, ops._stream()))
    else:
        check(lib().dtk_vit_attention(*[ops._p(t) for t in dev], ops._p(outs[0]), F, H, S, Sp,
                                      ot | (OPERAND_ATTENTION_V4 if kernel == "v4" else 0), ops._stream()))
    torch.cuda.synchronize()
    for b in bufs:
        b = b.cpu()
        assert (b[:guard] == SENTINEL).all() and (b[guard + n:] == SENTINEL).all(), "a store outside out[F][S][H * 64]"
    got = sum(o.double().cpu() for o in outs)
    rel = R.row_rel(got, ref)
    # the worst (frame, head, query): the head whose 64 outputs hold the row's largest error
    f, r = divmod(int(torch.nan_to_num(rel, nan=float("inf")).argmax()), S)
    h = int((got[f, r] - ref[f, r]).abs().nan_to_num(nan=float("inf")).view(H, 64).amax(dim=-1).argmax())
    worst = dict(frame=f, head=h, query=r, tag=R.tag_of(crafted, f, h, r), rel=rel[f, r].item())
    print(f"{kernel} {dt} {R.shape_id(shape)} {pads}: max row-relative error {worst['rel']:.2e} at {worst}")
    assert torch.isfinite(got).all(), worst
    assert rel.max().item() < (R.TOL["split", dt] if split else R.fast_bound(dt, S)), worst
