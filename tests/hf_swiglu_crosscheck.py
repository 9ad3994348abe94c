"""Standalone cross-check of tests/vitg_ref.vitg_block (the SwiGLU block restated in float64) against transformers' Dinov2 layer with
use_swiglu_ffn=True (Dinov2SwiGLUFFN: weights_in = w12, weights_out = w3), random weights mapped across.  Pattern: hf_crosscheck.py."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import transformers as tr
from transformers.models.dinov2.modeling_dinov2 import Dinov2SwiGLUFFN
import vitg_ref as G
cfg = tr.Dinov2Config(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, mlp_ratio=4, image_size=28, patch_size=14,
                      layerscale_value=1.0, use_swiglu_ffn=True)
hf = tr.Dinov2Model(cfg).eval()
g = torch.Generator().manual_seed(0)
sd = {}
for i, layer in enumerate(hf.encoder.layer):
    assert isinstance(layer.mlp, Dinov2SwiGLUFFN)
    p = f"blocks.{i}."
    for prm in layer.parameters():
        prm.data = torch.randn(prm.shape, generator=g) * 0.1
    att = layer.attention.attention
    sd[p + "norm1.weight"], sd[p + "norm1.bias"] = layer.norm1.weight.data, layer.norm1.bias.data
    sd[p + "attn.qkv.weight"] = torch.cat([att.query.weight.data, att.key.weight.data, att.value.weight.data])
    sd[p + "attn.qkv.bias"] = torch.cat([att.query.bias.data, att.key.bias.data, att.value.bias.data])
    sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"] = layer.attention.output.dense.weight.data, layer.attention.output.dense.bias.data
    sd[p + "ls1.gamma"], sd[p + "ls2.gamma"] = layer.layer_scale1.lambda1.data, layer.layer_scale2.lambda1.data
    sd[p + "norm2.weight"], sd[p + "norm2.bias"] = layer.norm2.weight.data, layer.norm2.bias.data
    sd[p + "mlp.w12.weight"], sd[p + "mlp.w12.bias"] = layer.mlp.weights_in.weight.data, layer.mlp.weights_in.bias.data
    sd[p + "mlp.w3.weight"], sd[p + "mlp.w3.bias"] = layer.mlp.weights_out.weight.data, layer.mlp.weights_out.bias.data
assert sd["blocks.0.mlp.w12.weight"].shape == (2 * 176, 64)      # hidden = (int(256 * 2 / 3) + 7) // 8 * 8
x = torch.randn(1, 37, 64, generator=g)
with torch.no_grad():
    y = x
    for layer in hf.encoder.layer:
        y = layer(y)
        y = y[0] if isinstance(y, tuple) else y
    z = x.double()
    for i in range(2):
        z = G.vitg_block(z, G.to64(sd), i, heads=4)
err = (y.double() - z).abs().max().item()
print(f"vitg reference vs transformers Dinov2 SwiGLU layer: max |diff| = {err:.2e}")
assert err < 1e-4
