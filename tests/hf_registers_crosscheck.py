"""Standalone cross-check of tests/vitreg_ref.encode (the register encoder restated in float64) against transformers'
Dinov2WithRegistersModel: random weights mapped across, stride 14, a square image at the native position grid (42 x 42, 3 x 3 patches: the
model's own table, so neither side interpolates -- vitreg_ref is handed the table through pos_rows), a tiny config with four registers.
Compared: the last hidden state BEFORE the final norm (hidden_states[-1]), all 1 + 4 + 9 rows.  Pattern: hf_swiglu_crosscheck.py."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import transformers as tr
import vitreg_ref as V
cfg = tr.Dinov2WithRegistersConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, mlp_ratio=4, image_size=42, patch_size=14,
                                   layerscale_value=1.0, num_register_tokens=4)
hf = tr.Dinov2WithRegistersModel(cfg).eval()
g = torch.Generator().manual_seed(0)
for prm in hf.parameters():
    prm.data = torch.randn(prm.shape, generator=g) * 0.1
emb = hf.embeddings
sd = {"cls_token": emb.cls_token.data, "pos_embed": emb.position_embeddings.data, "register_tokens": emb.register_tokens.data,
      "patch_embed.proj.weight": emb.patch_embeddings.projection.weight.data, "patch_embed.proj.bias": emb.patch_embeddings.projection.bias.data}
assert sd["register_tokens"].shape == (1, 4, 64) and sd["pos_embed"].shape == (1, 10, 64)
for i, layer in enumerate(hf.encoder.layer):
    p = f"blocks.{i}."
    att = layer.attention.attention
    sd[p + "norm1.weight"], sd[p + "norm1.bias"] = layer.norm1.weight.data, layer.norm1.bias.data
    sd[p + "attn.qkv.weight"] = torch.cat([att.query.weight.data, att.key.weight.data, att.value.weight.data])
    sd[p + "attn.qkv.bias"] = torch.cat([att.query.bias.data, att.key.bias.data, att.value.bias.data])
    sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"] = layer.attention.output.dense.weight.data, layer.attention.output.dense.bias.data
    sd[p + "ls1.gamma"], sd[p + "ls2.gamma"] = layer.layer_scale1.lambda1.data, layer.layer_scale2.lambda1.data
    sd[p + "norm2.weight"], sd[p + "norm2.bias"] = layer.norm2.weight.data, layer.norm2.bias.data
    sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = layer.mlp.fc1.weight.data, layer.mlp.fc1.bias.data
    sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = layer.mlp.fc2.weight.data, layer.mlp.fc2.bias.data
x = torch.randn(2, 3, 42, 42, generator=g)
with torch.no_grad():
    y = hf(pixel_values=x, output_hidden_states=True).hidden_states[-1]
    sd64 = V.to64(sd)
    z = V.encode(x.double(), sd64, 1, heads=4, stride=14, normalize=False, pos_rows=sd64["pos_embed"])["tokens"]
assert y.shape == z.shape == (2, 14, 64)
err = (y.double() - z).abs().max().item()
rel = ((y.double() - z).norm() / z.norm()).item()
print(f"vitreg reference vs transformers Dinov2WithRegistersModel (before the final norm): max |diff| = {err:.2e}, rel {rel:.2e}")
# float32 (transformers) against float64: the level hf_swiglu_crosscheck.py records (4e-7) is float32's own rounding over two blocks; 2e-6
# leaves the factor 4 that tests/test_vitreg_reference.py leaves the float32 oracle.  A row out of place, a register with a position row or
# a missing register is O(0.1) relative here
assert rel < 2e-6
