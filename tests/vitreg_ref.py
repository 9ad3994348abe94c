"""DINOv2 with registers (dinov2_vit{s,b,l,g}14_reg) -- the reference of the tests that cover it: tests/test_vitreg_reference.py (CPU)
and tests/test_gpu_vitreg.py.

The encoder restated in plain torch (float64 when the inputs are), from upstream's prepare_tokens_with_masks with
R = num_register_tokens:

    row 0          cls_token + pos_embed[0]
    rows 1 .. R    register_tokens[0 .. R-1]                      (no position encoding: inserted after it is added)
    rows 1+R ..    patch tokens + interpolated pos_embed[1:]      (row-major over the ph x pw grid)

Patch embedding at any stride; positions by `_fix_pos_enc`'s arithmetic at every stride (oracle.ref_algo.vit_pos_embed: the project does
not reproduce upstream's own anti-aliased interpolation at stride == patch, docs/PARITY.md); blocks with the GELU MLP (ViT-S / B / L) or
the SwiGLU feed-forward (ViT-g: tests/vitg_ref.swiglu_ffn), chosen by the keys of the state dict.  A state dict without
`register_tokens` is the plain model (R = 0).  Independent of VitExtractor: nothing here imports it.

`encode` returns the records the device returns -- tokens / qkv [B, 1+R+HW, .], features [B, HW, D] -- and can plant one defect of the
kind a device implementation could have (DEFECTS).  `check` is the comparison of the GPU tests; test_vitreg_reference.py shows that it
accepts a float32 run of this restatement and rejects every planted defect.
"""
import functools

import torch
import torch.nn.functional as F

from dino_tracker_amd import synth
from oracle import ref_algo
from vitg_ref import swiglu_ffn, to64  # noqa: F401  (to64: re-exported for the tests)

# the project's tolerance classes (tests/test_gpu_p1.py, tests/test_gpu_vitg.py, docs/PARITY.md)
FP16_TOL = dict(cos_min=0.999999, rel_max=8e-4)     # fast fp16 operands at LayerScale 1.0
BF16_TOL = dict(cos_min=0.999, rel_max=2e-2)        # fast bf16 operands
SPLIT_FACTOR = 4.0                                  # split operands: <= 4 x the float32 restatement's own error against float64

DEFECTS = ("reg_pos",        # the registers are given a position-encoding row (the first R patch rows of the interpolated table)
           "reg_after",      # the registers are placed after the patches instead of behind CLS
           "drop_cls_only",  # the prefix drop is off by the registers: rows 1 .. 1+HW are returned as features
           "keep_one_reg",   # CLS and R - 1 registers dropped, one register kept: rows R .. R+HW are returned as features
           "reg_zero")       # the register rows are zero


def n_registers(sd):
    return int(sd["register_tokens"].shape[1]) if "register_tokens" in sd else 0


def without_registers(sd):
    return {k: v for k, v in sd.items() if k != "register_tokens"}


def block(x, sd, i, heads, return_qkv=False):
    """DINOv2 block at eval: x += g1 proj(MHSA(LN1 x)); x += g2 ffn(LN2 x); LN eps 1e-6; softmax(q k^T / sqrt(d_head)) spelled out."""
    p = f"blocks.{i}."
    b, s, d = x.shape
    y = F.layer_norm(x, (d,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps=1e-6)
    qkv_flat = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
    q, k, v = qkv_flat.reshape(b, s, 3, heads, d // heads).permute(2, 0, 3, 1, 4)
    a = torch.softmax((q @ k.transpose(-1, -2)) * (q.shape[-1] ** -0.5), dim=-1) @ v
    a = a.transpose(1, 2).reshape(b, s, d)
    x = x + sd[p + "ls1.gamma"] * F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    y = F.layer_norm(x, (d,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps=1e-6)
    if p + "mlp.w12.weight" in sd:
        y = swiglu_ffn(y, sd, p)
    else:
        y = F.linear(F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    out = x + sd[p + "ls2.gamma"] * y
    return (out, qkv_flat) if return_qkv else out


def embed(frames, sd, stride=7, patch=14, normalize=True, pos_rows=None, defect=None):
    """frames [B,3,H,W] -> the token rows before the first block, [B, 1+R+HW, D].  pos_rows [1, 1+HW, D]: the position table to add
    instead of the interpolated one (the cross-check against transformers runs at the native grid, where neither side interpolates)."""
    x = frames
    if normalize:
        m = torch.tensor(ref_algo.IMAGENET_MEAN, dtype=frames.dtype).view(1, 3, 1, 1)
        s = torch.tensor(ref_algo.IMAGENET_STD, dtype=frames.dtype).view(1, 3, 1, 1)
        x = (x - m) / s
    ph, pw = ref_algo.feature_grid(frames.shape[-2], frames.shape[-1], patch, stride)
    tok = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=stride).flatten(2).transpose(1, 2)
    b = tok.shape[0]
    pos = ref_algo.vit_pos_embed(sd, ph, pw) if pos_rows is None else pos_rows
    tok = torch.cat([sd["cls_token"].expand(b, -1, -1), tok], dim=1) + pos
    if n_registers(sd):
        reg = sd["register_tokens"].expand(b, -1, -1)
        if defect == "reg_pos":
            reg = reg + pos[:, 1:1 + reg.shape[1]]
        if defect == "reg_zero":
            reg = torch.zeros_like(reg)
        parts = (tok[:, :1], tok[:, 1:], reg) if defect == "reg_after" else (tok[:, :1], reg, tok[:, 1:])
        tok = torch.cat(parts, dim=1)
    return tok


def encode(frames, sd, layer, heads, stride=7, patch=14, normalize=True, pos_rows=None, defect=None, taps=None):
    """The records of block `layer` (-1: the embedding only) for frames [B,3,H,W], in the dtype of frames / sd:
    {"tokens" [B, 1+R+HW, D], "qkv" [B, 1+R+HW, 3D] (None for layer -1), "feat" [B, HW, D]: the tokens without CLS and the registers,
    "taps": the mean of the outputs of the blocks in `taps`}."""
    tok = embed(frames, sd, stride, patch, normalize, pos_rows, defect)
    r = n_registers(sd)
    hw = tok.shape[1] - 1 - r
    qkv, acc = None, None
    for i in range(layer + 1):
        tok, qkv = block(tok, sd, i, heads, return_qkv=True)
        if taps is not None and i in taps:
            acc = tok / len(taps) if acc is None else acc + tok / len(taps)
    first = {"drop_cls_only": 1, "keep_one_reg": r}.get(defect, 1 + r)
    return {"tokens": tok, "qkv": qkv, "feat": tok[:, first:first + hw], "taps": acc}


def rel(got, ref):
    return float((got.double().cpu() - ref.double()).norm() / ref.double().norm())


def check(got, ref, cos_min, rel_max):
    """The comparison of the GPU tests: per-row cosine >= cos_min and relative Frobenius error <= rel_max; returns (min cos, rel)."""
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "non-finite output"
    cos = F.cosine_similarity(got, ref, dim=-1)
    r = (got - ref).norm() / ref.norm()
    assert cos.min() >= cos_min, f"min row cosine {cos.min().item():.7f} < {cos_min} (rel {r.item():.2e})"
    assert r <= rel_max, f"relative Frobenius error {r.item():.2e} > {rel_max:.2e} (min row cosine {cos.min().item():.7f})"
    return cos.min().item(), r.item()


def check_split(got, ref, ref32):
    """Split operands: relative Frobenius error <= SPLIT_FACTOR x that of the float32 restatement `ref32` (docs/PARITY.md, the RAFT rule)."""
    r, r32 = rel(got, ref), rel(ref32, ref)
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert r <= SPLIT_FACTOR * r32, f"relative Frobenius error {r:.2e} > {SPLIT_FACTOR:g} x {r32:.2e} (float32 restatement)"
    return r, r32


def check_records(got, ref, cos_min, rel_max, records=("tokens", "feat", "qkv")):
    """`check` on every record of one encode: what the GPU tests assert of a fast pass.  Returns {record: (min cos, rel)}."""
    return {k: check(got[k], ref[k], cos_min, rel_max) for k in records}


def check_embedding_exact(tokens, plain_tokens, register_tokens):
    """The exact comparison (layer -1: patch embedding and positions, no block): CLS row and patch rows bit-equal to the plain sibling's on
    the same weights, register rows bit-equal to register_tokens."""
    r = register_tokens.shape[1]
    tokens, plain_tokens = tokens.cpu(), plain_tokens.cpu()
    assert tokens.shape[1] == plain_tokens.shape[1] + r, (tuple(tokens.shape), tuple(plain_tokens.shape))
    assert torch.equal(tokens[:, 0], plain_tokens[:, 0]), "row 0 (CLS + its position) differs from the plain model's"
    assert torch.equal(tokens[:, 1:1 + r], register_tokens.to(tokens.dtype).expand(tokens.shape[0], -1, -1)), "rows 1 .. R are not register_tokens"
    assert torch.equal(tokens[:, 1 + r:], plain_tokens[:, 1:]), "rows 1 + R .. differ from the plain model's patch rows"


# ---- the cases of the GPU tests (tests/test_gpu_vitreg.py), shared with the CPU test that asserts their sensitivity to the registers ----
SEED_WEIGHTS, SEED_VIDEO = 9, 73
CASES = {   # key: (model, (frames, H, W), stride, last block)
    "main": ("dinov2_vits14_reg", (3, 98, 126), 7, 1),       # 13 x 17 patches, S = 226: frame ends inside every row tile
    "main14": ("dinov2_vits14_reg", (3, 98, 126), 14, 1),    # the generic patch embedding: 7 x 9 patches, S = 68
    "sp": ("dinov2_vits14_reg", (2, 42, 182), 7, 1),         # 5 x 25 = 125 patches: S = 130, Sp = 256 (the plain model: 126, 128)
    "short": ("dinov2_vits14_reg", (3, 28, 42), 7, 1),       # 15 patches, S = 20 < 32 with several frames
    "one": ("dinov2_vits14_reg", (1, 14, 14), 7, 1),         # one patch, S = 6
    "vitb": ("dinov2_vitb14_reg", (3, 98, 126), 7, 0),
    "vitl": ("dinov2_vitl14_reg", (3, 98, 126), 7, 0),
    "vitg": ("dinov2_vitg14_reg", (3, 98, 126), 7, 0),
}


@functools.lru_cache(maxsize=None)
def make_case(key):
    """Weights (the first blocks, LayerScale 1.0), frames and the CPU references of one case, computed once per process:
    ref[l] = the float64 records of block l, ref32 = the float32 run of the last block (the yardstick of the split path)."""
    name, shape, stride, last = CASES[key]
    heads = synth.VIT_CONFIGS[name]["heads"]
    sd = synth.make_vit_weights(name, seed=SEED_WEIGHTS, nblocks=last + 1)
    video = synth.synth_video(*shape, seed=SEED_VIDEO)
    sd64 = to64(sd)
    with torch.no_grad():
        ref = {l: encode(video.double(), sd64, l, heads, stride=stride, taps=tuple(range(l + 1))) for l in range(last + 1)}
        ref32 = encode(video, sd, last, heads, stride=stride)
    return {"name": name, "plain": name[:-len("_reg")], "sd": sd, "sd64": sd64, "video": video, "stride": stride, "layer": last, "heads": heads,
            "ref": ref, "ref32": ref32}


def register_sensitivity(key):
    """Relative Frobenius distance of the float64 patch features of a case's last block between "with registers" and "registers removed"."""
    c = make_case(key)
    with torch.no_grad():
        plain = encode(c["video"].double(), without_registers(c["sd64"]), c["layer"], c["heads"], stride=c["stride"])
    return rel(plain["feat"], c["ref"][c["layer"]]["feat"])
