"""CPU helper of the stand-alone attention tests (dtk_vit_attention, dtk_vit_attention_split): operands with crafted rows at any
token count, the float64 reference on the operands actually passed, and the per-row error metric.  No GPU import.

The kernels work in the exp2 domain: q arrives multiplied by log2(e) / sqrt(64), the reference is softmax(s ln 2) v with s = q k^T.

SHAPES is the table tests/test_gpu_vit_attention_shapes.py runs and tests/test_vit_attention_reference.py checks the builder on; the
seed of a shape is part of the table: the builder's claims about its crafted rows (below) are conditions on the random draw, the CPU
test asserts them for exactly these seeds, in fp32 and after rounding to fp16 / bf16.  (Each seed is the smallest one from 1 for which
they hold: "every score of an all-negative row below -20" trims the tail of one key channel of one head, which is rare at 700 keys.)"""
import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
QS = 0.125 * LOG2E              # log2(e) / sqrt(64)

# (S, Sp, F, H, seed); ntiles = ceil(S / 64)
SHAPES = [
    (1, 64, 1, 1, 1),       # one key and one query: the output is that key's value row
    (33, 64, 1, 2, 1),      # one tile with a tail; the second 32-query tile holds one valid row
    (64, 64, 1, 2, 2),      # one tile, no tail, Sp == S (a 56 x 70 frame at stride 7)
    (65, 128, 3, 3, 2),     # two tiles, a one-key tail; F H = 9
    (128, 128, 1, 2, 1),    # two tiles, no tail
    (129, 256, 1, 2, 3),    # three tiles = the prologue's requests; a whole padding tile; one valid row in the second 128 queries
    (222, 256, 1, 6, 3),    # four tiles = one turn of the ring
    (257, 320, 1, 2, 3),    # five tiles; one valid row in the second 256 queries
    (320, 320, 1, 12, 2),   # five tiles, no tail; F H = 12
    (384, 384, 1, 2, 27),   # six tiles, no tail
    (513, 576, 3, 3, 289),  # one valid row in the second 512 queries; QB = 2 with F H = 9
    (577, 640, 1, 2, 119),  # ten tiles (% 4 == 2) with a tail
    (705, 768, 2, 5, 63),   # twelve tiles (% 4 == 0), a one-key tail; F H = 10
]


# Bounds on row_rel.max(): those of the two existing stand-alone tests (tests/test_gpu_p1.py::test_attention_guards_and_safe_pass,
# tests/test_gpu_precision.py::test_attention_stage_on_split_operands) for the same metric.
TOL = {("fast", "fp16"): 1e-3, ("fast", "bf16"): 6e-3, ("split", "fp16"): 2e-5, ("split", "bf16"): 4e-3}
# The cases in which the two roundings a 16-bit kernel cannot avoid, emulated in float64 from the operands (emulated_16bit below),
# are ALONE beyond the bound: (type, S) -> the emulated row_rel.max().  bf16 has 8 significant bits: P and the output are each
# rounded by up to 2^-8 = 3.9e-3 and 6e-3 is 1.5 of those, not a worst case.  The fast kernels are held to TWICE the emulated figure in
# these cases (test_vit_attention_reference.py asserts that this table is exactly the set of cases whose emulation exceeds TOL).
EMULATED_BEYOND_TOL = {("bf16", 222): 6.655e-3, ("bf16", 320): 6.084e-3, ("bf16", 384): 7.090e-3, ("bf16", 577): 7.141e-3}


def fast_bound(dt, S):
    """The bound of a dtk_vit_attention case: TOL, or twice the emulated format error where that alone exceeds TOL."""
    e = EMULATED_BEYOND_TOL.get((dt, S))
    return TOL["fast", dt] if e is None else 2.0 * e


def shape_id(shape):
    S, Sp, F, H, _ = shape
    return f"S{S}-Sp{Sp}-{F}x{H}"


def make_case(S, Sp, F, H, seed, pads):
    """fp32 q (exp2 domain), k, v, each [F][H][Sp][64], and the crafted rows as a list of (frame, head, row, tag).

    Rows 0 .. S-1: randn, q scaled by 1.5 QS.  Rows S .. Sp-1 (the padding rows of Q and K, the padding columns of V^T):
    pads = "zero": 0; pads = "finite": uniform in [-3, 3], from a generator of their own -- the valid rows are the same in both modes.

    Crafted rows, each only where the shape has room for it:
      * "all-negative": head 0 of frame 0, +8 on channel 0 of every valid key and q[..., 0] = -4 for the rows 0, S - 1 and (S > 32)
        S - 33: every score of these rows is about -32, so ONE unmasked padding key (score 0 with zero pads) would take the whole
        softmax;
      * "sharp": the last valid row of the last head of the last frame times 120: scores of hundreds, the row goes to the safe pass,
        in the wave that straddles S.  (F = H = 1: this is the all-negative row S - 1 as well; it keeps both properties and both tags);
      * "late-tile" (ntiles >= 2): head H - 1 of frame 0, +20 on channel 1 of the keys of the LAST key tile, and row 0 = 0.05 q with
        q[1] = 2: scores about 0 before the last tile and about +40 in it, so the guard trips on the last tile and is still pending when
        the key loop ends.  (H = 1 would put this in head 0 next to the +8 shift of channel 0; row 0 would then carry both tags.  No
        shape of the table has H = 1 and two tiles.)"""
    assert pads in ("zero", "finite") and 1 <= S <= Sp and Sp % 64 == 0
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(F, H, Sp, 64)
    k = torch.zeros(F, H, Sp, 64)
    v = torch.zeros(F, H, Sp, 64)
    q[:, :, :S] = torch.randn(F, H, S, 64, generator=g) * QS * 1.5
    k[:, :, :S] = torch.randn(F, H, S, 64, generator=g)
    v[:, :, :S] = torch.randn(F, H, S, 64, generator=g)
    if pads == "finite" and Sp > S:
        gp = torch.Generator().manual_seed(seed + 7919)
        for x in (q, k, v):
            x[:, :, S:] = torch.rand(F, H, Sp - S, 64, generator=gp) * 6.0 - 3.0
    ntiles = (S + 63) // 64
    crafted = []
    k[0, 0, :S, 0] += 8.0
    for r in sorted({0, S - 1} | ({S - 33} if S > 32 else set())):
        q[0, 0, r, 0] = -4.0
        crafted.append((0, 0, r, "all-negative"))
    q[F - 1, H - 1, S - 1] *= 120.0
    crafted.append((F - 1, H - 1, S - 1, "sharp"))
    if ntiles >= 2:
        k[0, H - 1, 64 * (ntiles - 1):S, 1] += 20.0
        q[0, H - 1, 0] *= 0.05
        q[0, H - 1, 0, 1] = 2.0
        crafted.append((0, H - 1, 0, "late-tile"))
    return q, k, v, crafted


def scores(qb, kb, S):
    """float64 exp2-domain scores [F][H][S][S] of the valid rows of the operands as passed."""
    return qb.double()[:, :, :S] @ kb.double()[:, :, :S].transpose(2, 3)


def reference(qb, kb, vb, S):
    """float64 softmax(s ln 2) v on the operands actually passed (q, k, v [F][H][Sp][64], any float type; rows S .. are not read):
    [F][S][H * 64], the layout of the kernels' output."""
    F, H = qb.shape[0], qb.shape[1]
    p = torch.softmax(scores(qb, kb, S) * LN2, dim=-1)
    return (p @ vb.double()[:, :, :S]).permute(0, 2, 1, 3).reshape(F, S, H * 64)


def row_rel(got, ref):
    """Per (frame, query): the largest absolute error over the row's H * 64 outputs, relative to the row's largest |reference|
    (at least 0.05): [F][S]."""
    err = (got.double() - ref).abs().amax(dim=-1)
    return err / ref.abs().amax(dim=-1).clamp(min=0.05)


def emulated_16bit(qb, kb, vb, S, tdt, against="estimate"):
    """The same product with the two roundings a 16-bit attention kernel cannot avoid, everything else in float64: P = 2^(s - m)
    rounded to `tdt` before the PV product (the row sum takes the unrounded P, as the kernels' does) and the output rounded to `tdt`.
    What row_rel(emulated_16bit(...), reference(...)) shows is the error inherent to the format for these operands; it is computed
    from the operands alone, never from a kernel's output.

    Any m gives the same softmax, but WHERE the values of P fall on the 16-bit mantissa grid depends on the fractional part of m, and
    with it the rounding error of a row (not its size class: its sample).  against="estimate": m is the reference the fast kernels
    document (csrc/vit_attention_common.h, "the guard arithmetic"): the row's largest score over the first 64 keys and over the 32
    keys of its own query tile, moved by whole binades only (a power-of-two rescale leaves the mantissas alone; here: by
    floor(row maximum - estimate), which keeps the float64 exponentials in range).  against="max": m is the row maximum."""
    F, H = qb.shape[0], qb.shape[1]
    s = scores(qb, kb, S)
    m = s.amax(dim=-1, keepdim=True)
    if against == "estimate":
        idx = torch.arange(S)
        seen = (idx[None, :] < 64) | ((idx[:, None] // 32) == (idx[None, :] // 32))
        est = s.masked_fill(~seen, float("-inf")).amax(dim=-1, keepdim=True)
        m = est + torch.floor(m - est)
    else:
        assert against == "max"
    p = torch.exp2(s - m)
    o = (p.to(tdt).double() @ vb.double()[:, :, :S]) / p.sum(dim=-1, keepdim=True)
    return o.to(tdt).double().permute(0, 2, 1, 3).reshape(F, S, H * 64)


def tag_of(crafted, f, h, row):
    """The tags of (frame, head, row), or "plain"."""
    tags = [t for (cf, ch, cr, t) in crafted if (cf, ch, cr) == (f, h, row)]
    return "+".join(tags) if tags else "plain"


def crafted_row_claims(q, k, S, crafted):
    """What make_case promises about its crafted rows, measured on the given (possibly rounded) q and k: a list of
    (tag, (frame, head, row), holds, figures)."""
    s = scores(q, k, S)
    ntiles = (S + 63) // 64
    out = []
    for f, h, r, tag in crafted:
        row = s[f, h, r]
        if tag == "all-negative":
            fig = (row.max().item(),)
            ok = fig[0] < -20
        elif tag == "sharp":
            fig = (row.abs().max().item(),)
            ok = fig[0] > 150
        else:
            last0 = 64 * (ntiles - 1)
            fig = (row[last0:].min().item(), row[:min(S, 96, last0)].max().item())
            ok = fig[0] > 30 and fig[1] < 8
        out.append((tag, (f, h, r), ok, fig))
    return out
