"""Same-box A / B of the stand-alone attention stage between two builds of libdtk.so (ctypes handles of both in one process):
    python scripts/attn_ab.py <lib A>[:flags] <lib B>[:flags] [<lib C>[:flags] ...]      (flags: OR-ed into operand_type: 0x2000 =
    DTK_OPERAND_ATTENTION_V4, the attention4 kernel; none = attention6.  A current library refuses every other bit.)
Benchmark shapes (frames x 6 heads, S = 8108, random fp16 operands), alternating blocks of launches, hipEvents around each block."""
import ctypes
import sys

import torch

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from dino_tracker_amd._lib import SIGNATURES  # noqa: E402


def load(path):
    h = ctypes.CDLL(path)
    res, args = SIGNATURES["dtk_vit_attention"]
    h.dtk_vit_attention.restype, h.dtk_vit_attention.argtypes = res, args
    return h


def main():
    specs = [x for x in sys.argv[1:] if not x.isdigit()]
    T = int([x for x in sys.argv[1:] if x.isdigit()][0]) if any(x.isdigit() for x in sys.argv[1:]) else 90
    libs = []
    for sp in specs:
        path, _, fl = sp.partition(":")
        libs.append((sp, load(path), int(fl, 0) if fl else 0))
    heads, S = 6, 67 * 121 + 1
    Sp = (S + 127) // 128 * 128
    g = torch.Generator(device="cuda").manual_seed(5)
    q = (torch.randn(T, heads, Sp, 64, device="cuda", generator=g) * (0.125 * 1.4426950408889634)).half()
    k = torch.randn(T, heads, Sp, 64, device="cuda", generator=g).half()
    v = torch.randn(T, heads, 64, Sp, device="cuda", generator=g).half()
    k[:, :, S:] = 0
    v[:, :, :, S:] = 0
    outs = [torch.full((T, S, heads * 64), float("nan"), dtype=torch.float16, device="cuda") for _ in libs]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(i):
        _, h, fl = libs[i]
        rc = h.dtk_vit_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), outs[i].data_ptr(), T, heads, S, Sp, fl, st)
        assert rc == 0, (rc, libs[i][0])
    for i in range(len(libs)):
        for _ in range(3):
            run(i)
    torch.cuda.synchronize()
    for i in range(1, len(libs)):
        d = (outs[i].float() - outs[0].float()).abs()
        print(f"{libs[i][0]} vs {libs[0][0]}: bit-identical {bool(torch.equal(outs[i], outs[0]))}, max |diff| {float(d.max()):.3e} "
              f"(max |ref| {float(outs[0].float().abs().max()):.3e}), finite {bool(torch.isfinite(outs[i]).all())}")
    # accuracy of every variant against a float64 softmax on the SAME 16-bit operands (frame 0, all heads, 512 queries spread over S)
    rows = torch.linspace(0, S - 1, 512, device="cuda").long()
    sc64 = q[0, :, rows].double() @ k[0, :, :S].double().transpose(1, 2)                 # [heads, 512, S], exp2 domain
    p64 = torch.softmax(sc64 * 0.6931471805599453, dim=-1)
    ref = (p64 @ v[0, :, :, :S].double().transpose(1, 2)).permute(1, 0, 2).reshape(512, heads * 64)
    for i in range(len(libs)):
        got = outs[i][0, rows].double()
        err = got - ref
        print(f"{libs[i][0]}: vs float64 on the same operands: rel Frobenius {float(err.norm() / ref.norm()):.3e}, "
              f"max |err| {float(err.abs().max()):.3e}, mean signed err / mean |ref| {float(err.mean() / ref.abs().mean()):+.2e}")
    res = {i: [] for i in range(len(libs))}
    for rnd in range(6):
        for i in range(len(libs)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                run(i)
            e1.record()
            torch.cuda.synchronize()
            res[i].append(e0.elapsed_time(e1) / 10)
    fl = 4.0 * S * S * 384 * T
    for i in range(len(libs)):
        ms = sorted(res[i])
        med = ms[len(ms) // 2]
        print(f"{libs[i][0]}: median {med:.4f} ms per launch ({fl / med / 1e9:.1f} TFLOP/s), blocks {[round(x, 3) for x in res[i]]}")


if __name__ == "__main__":
    main()
