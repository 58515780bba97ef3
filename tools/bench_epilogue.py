"""Time the ViT-B linears of the headline step (qkv, fc1 operand-out; proj, fc2 fp32-out with bias, LayerScale and residual) and one
Winograd F(4x4, 3x3) convolution on a pinned tile, under the library PP_LIB_SUFFIX selects (shipped / -DPP_STUDY_NOSTORE /
-DPP_STUDY_NOEPI study builds, or the generic epilogue body with GENERIC=1).  usage: bench_epilogue.py [M]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from picopose_amd import _lib, ops  # noqa: E402

M = int(sys.argv[1]) if len(sys.argv) > 1 else 49344
d = "cuda"
tag = os.environ.get("PP_LIB_SUFFIX", "") or "shipped"
L = _lib.lib()
if os.environ.get("GENERIC") == "1":
    L.pp_gemm_generic_epilogue(1)
    tag += "+generic"
g = torch.Generator().manual_seed(0)


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


with torch.no_grad():
    res = torch.randn(M, 768, generator=g).to(d)
    gam = torch.rand(768, generator=g).to(d)
    for name, K, N, cfg, kw in [("qkv", 768, 2304, 5, dict(out_split=True)), ("fc1", 768, 3072, 5, dict(act="gelu", out_split=True)),
                                ("proj", 768, 768, 4, dict(gamma=gam, residual=res)), ("fc2", 3072, 768, 4, dict(gamma=gam, residual=res))]:
        x = torch.randn(M, K, generator=g).to(d)
        w = (torch.randn(N, K, generator=g) / K ** 0.5).to(d)
        b = torch.randn(N, generator=g).to(d)
        xs = ops.Split(ops.split_activation(x, 1, M, K, 0, K))
        os.environ["PP_GEMM_FORCE_CFG"] = str(cfg)
        ms = timed(lambda: ops.linear(xs, w, b, **kw))
        print(f"{tag:16s} {name:5s} M={M} N={N} K={K} cfg={cfg} {ms:.3f} ms {2 * M * N * K / ms / 1e9:.0f} TFLOP/s useful", flush=True)
    # a Winograd F(4x4, 3x3) convolution of the heads (transforms included; its 36 dense products are one grouped launch)
    B, hw, cin, cout = 32, 32, 256, 256
    x = torch.randn(B, hw, hw, cin, generator=g).to(d)
    wp = ops.pack_conv_weight((torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).to(d))
    bias = torch.randn(cout, generator=g).to(d)
    xs = ops.split_image(x)
    for cfg in (5, 4):
        os.environ["PP_GEMM_FORCE_CFG"] = str(cfg)
        ms = timed(lambda: ops.conv2d(xs, wp, bias, 3, pad=1, act="relu", wino=True))
        print(f"{tag:16s} wino4 B={B} {hw}x{hw} {cin}->{cout} cfg={cfg} {ms:.3f} ms (whole convolution)", flush=True)
