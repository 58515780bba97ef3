"""The 256x192 tile of the pre-split contraction kernel (PP_GEMM_FORCE_CFG=11): a new instantiation of the one K loop, so every output
element keeps the bits the 128x128 (cfg 0) and 256x256 (cfg 5) tiles give it — dense with row, column and K tails, 3x3 convolutions in
the channel-slice-major K order, a natural-order convolution at Cin = 8, fp32 and operand-only outputs, both operand formats — and
stays inside the float64 bound of tests/engine_bounds.py.  The launch records show that the tile really ran."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_bounds as eb  # noqa: E402

gpu = pytest.mark.gpu
CFG = 11


@pytest.fixture(params=["f16x3", "f16"])
def mode(request, monkeypatch):
    from picopose_amd import ops

    monkeypatch.setattr(ops, "PRECISION", request.param)
    monkeypatch.setattr(ops, "WINOGRAD4", False)          # the direct implicit-GEMM convolution
    monkeypatch.delenv("PP_GEMM_FORCE_CFG", raising=False)
    ops.saturation_raised()
    yield request.param
    ops.drop_split_cache()


def _pinned(fn, cfg):
    """fn() with PP_GEMM_FORCE_CFG = cfg -> (result, the configurations the engine's launch records name)."""
    from picopose_amd import _lib

    L, cap = _lib.lib(), 16
    old = os.environ.get("PP_GEMM_FORCE_CFG")
    os.environ["PP_GEMM_FORCE_CFG"] = str(cfg)
    _lib.check(L.pp_prof_gemm_enable(cap), "pp_prof_gemm_enable")
    try:
        out = fn()
        torch.cuda.synchronize()
        shape, ms = (ctypes.c_int * (8 * cap))(), (ctypes.c_float * cap)()
        fl, by, cnt = (ctypes.c_double * cap)(), (ctypes.c_double * cap)(), ctypes.c_int()
        _lib.check(L.pp_prof_gemm_records2(cap, shape, ms, fl, by, ctypes.byref(cnt)), "pp_prof_gemm_records2")
    finally:
        _lib.check(L.pp_prof_gemm_enable(0), "pp_prof_gemm_enable")
        os.environ.pop("PP_GEMM_FORCE_CFG", None) if old is None else os.environ.__setitem__("PP_GEMM_FORCE_CFG", old)
    return out, [(shape[8 * i + 4], shape[8 * i + 5], shape[8 * i + 6]) for i in range(cnt.value)]      # (cfg, kind, A-delivery mode)


def _bits(t):
    return t.hl.view(torch.int16) if hasattr(t, "hl") else t


def _three_tiles(fn, amode):
    """fn under cfg 11, 0 and 5 -> the cfg-11 result, after asserting that the 256x192 tile ran in `amode` and that all three agree bitwise."""
    got, recs = _pinned(fn, CFG)
    assert recs == [(CFG, 0, amode)], recs
    for other in (0, 5):
        ref, recs = _pinned(fn, other)
        assert [r[0] for r in recs] == [other], recs
        assert torch.equal(_bits(got), _bits(ref)), other
    return got


# M, N, K: N = 192 exactly; a part-filled second column tile; N = 136 (one part-filled tile); K = 288 (a K tail in the h format, 64 k per
# K tile) and 296 (a tail in the hl format too, 32 k per K tile); more than one tile row with a row tail
DENSE = [(300, 192, 256), (300, 200, 256), (300, 136, 256), (300, 192, 288), (300, 192, 296), (520, 384, 64)]


@gpu
@pytest.mark.parametrize("M,N,K", DENSE)
def test_dense_keeps_the_bits_of_the_other_tiles(mode, M, N, K):
    from picopose_amd import ops

    g = torch.Generator().manual_seed(M + N + K)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    xg, wg, bg, rg = x.cuda(), w.cuda(), b.cuda(), res.cuda()
    xs = ops.Split(ops.split_activation(xg, 1, M, K, 0, K))
    out = _three_tiles(lambda: ops.linear(xs, wg, bg, act="gelu", residual=rg), 0)                    # fp32 output
    _three_tiles(lambda: ops.linear(xs, wg, bg, act="relu", out_split=True), 0)                       # operand-only output
    if (N, K) in ((192, 256), (200, 256)):
        ref, bound = eb.reference("linear", x, w, mode, bias=b, act="gelu", residual=res)
        eb.check(f"256x192 linear {M}x{K}x{N}", out, ref, bound, mode)


@gpu
@pytest.mark.parametrize("B,H,W,cin,cout,k,amode", [
    (2, 16, 16, 256, 192, 3, 1),        # corr_net[1]'s layer: channel-slice-major K
    (1, 8, 24, 256, 192, 3, 1),         # a map narrower than a tile row block, one part-filled row tile
    (2, 12, 12, 8, 136, 7, 2),          # Cin = 8: natural K order (flow_net[0]'s kind of layer), K = 392: a K tail
])
def test_convolutions_keep_the_bits_of_the_other_tiles(mode, B, H, W, cin, cout, k, amode):
    from picopose_amd import ops

    g = torch.Generator().manual_seed(B * H + cin + cout)
    x = torch.randn(B, cin, H, W, generator=g)
    w, b = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, torch.randn(cout, generator=g)
    wp, bg = ops.pack_conv_weight(w.cuda()), b.cuda()
    xs = ops.split_image(ops.to_nhwc(x.cuda()))
    assert isinstance(xs, ops.Split)
    out = _three_tiles(lambda: ops.conv2d(xs, wp, bg, k, pad=k // 2, act="relu"), amode)
    _three_tiles(lambda: ops.conv2d(xs, wp, bg, k, pad=k // 2, act="relu", out_split=True, split_relu=True), amode)
    if (H, cin) == (16, 256):
        ref, bound = eb.reference("conv2d", x, w, mode, bias=b, act="relu", stride=1, padding=k // 2)
        eb.check("256x192 conv 256 -> 192", ops.to_nchw(out), ref, bound, mode)


