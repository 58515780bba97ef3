"""The specialised epilogue bodies of the pre-split kernel (csrc/pp_gemm_dev.h, PP_EPI_*) against its generic body: for every kind, on
both 256-wide tiles, on shapes with M and N tails, the outputs are bit for bit those of the generic body (pp_gemm_generic_epilogue(1))
and the saturation word ends up the same.  The launch records show that each run used the pinned tile."""
import ctypes
import os

import pytest
import torch

gpu = pytest.mark.gpu
TILES = [5, 4]                         # PP_GEMM_FORCE_CFG: 256x256, 256x128
SHAPES = [(1000, 776, 192), (49, 264, 96), (2100, 1032, 224)]   # (M, N, K): M and N tails on both tiles


def _records():
    from picopose_amd import _lib

    cap = 64
    shape, ms = (ctypes.c_int * (8 * cap))(), (ctypes.c_float * cap)()
    fl, by, cnt = (ctypes.c_double * cap)(), (ctypes.c_double * cap)(), ctypes.c_int()
    _lib.check(_lib.lib().pp_prof_gemm_records2(cap, shape, ms, fl, by, ctypes.byref(cnt)), "pp_prof_gemm_records2")
    return [dict(zip(("M", "N", "K", "k", "cfg", "kind", "amode"), (shape[8 * i + j] for j in range(7)))) for i in range(cnt.value)]


def run(fn, cfg, generic):
    """fn() on tile `cfg` with the generic (True) or the specialised epilogue -> (result, launch records, saturation raised)."""
    from picopose_amd import _lib, ops

    L = _lib.lib()
    old = os.environ.get("PP_GEMM_FORCE_CFG")
    os.environ["PP_GEMM_FORCE_CFG"] = str(cfg)
    assert L.pp_gemm_generic_epilogue(1 if generic else 0) == 0
    ops.saturation_raised()
    _lib.check(L.pp_prof_gemm_enable(64), "pp_prof_gemm_enable")
    try:
        out = fn()
        torch.cuda.synchronize()
        recs = _records()
    finally:
        _lib.check(L.pp_prof_gemm_enable(0), "pp_prof_gemm_enable")
        L.pp_gemm_generic_epilogue(0)
        if old is None:
            os.environ.pop("PP_GEMM_FORCE_CFG", None)
        else:
            os.environ["PP_GEMM_FORCE_CFG"] = old
    return out, recs, ops.saturation_raised()


def same(a, b):
    from picopose_amd import ops

    if isinstance(a, ops.Split):
        return torch.equal(a.hl, b.hl)
    return torch.equal(a, b)


@pytest.fixture
def f16x3(monkeypatch):
    from picopose_amd import ops

    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    monkeypatch.delenv("PP_GEMM_FORCE_CFG", raising=False)
    yield
    ops.drop_split_cache()


@gpu
@pytest.mark.parametrize("cfg", TILES)
@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("kind", ["hl_lin", "hl_gelu", "c_bgr", "c_plain"])
@torch.no_grad()
def test_epilogue_kind_equals_generic_body(f16x3, kind, M, N, K, cfg):
    from picopose_amd import ops

    g = torch.Generator().manual_seed(M + N + K + cfg)
    x = (torch.randn(M, K, generator=g) * 2.0).cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    b = torch.randn(N, generator=g).cuda()
    gam = (torch.rand(N, generator=g) + 0.1).cuda()
    res = torch.randn(M, N, generator=g).cuda()
    xs = ops.Split(ops.split_activation(x, 1, M, K, 0, K))
    fn = {
        "hl_lin": lambda: ops.linear(xs, w, b, out_split=True),
        "hl_gelu": lambda: ops.linear(xs, w, b, act="gelu", out_split=True),
        "c_bgr": lambda: ops.linear(xs, w, b, gamma=gam, residual=res),
        "c_plain": lambda: ops.linear(xs, w, None),
    }[kind]
    spec, rs, sat_s = run(fn, cfg, generic=False)
    gen, rg, sat_g = run(fn, cfg, generic=True)
    assert isinstance(spec, ops.Split) == kind.startswith("hl")
    assert [r["cfg"] for r in rs] == [cfg] and [r["cfg"] for r in rg] == [cfg], (rs, rg)
    assert [r["amode"] for r in rs] == [0]
    assert same(spec, gen), kind
    assert not sat_s and not sat_g


@gpu
@pytest.mark.parametrize("cfg", TILES)
@pytest.mark.parametrize("act", [None, "gelu"])
@torch.no_grad()
def test_operand_kinds_report_saturation_like_the_generic_body(f16x3, act, cfg):
    """Outputs beyond the operand range: the clamped operand and the saturation word agree with the generic body."""
    from picopose_amd import ops

    M, N, K = 600, 520, 128
    g = torch.Generator().manual_seed(7 + cfg)
    x = torch.randn(M, K, generator=g).cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    b = torch.randn(N, generator=g)
    b[::5] = 4.0e4                                          # every fifth column lands past the fp16 range of the 4x operand
    b = b.cuda()
    xs = ops.Split(ops.split_activation(x, 1, M, K, 0, K))
    fn = lambda: ops.linear(xs, w, b, act=act, out_split=True)  # noqa: E731
    spec, _, sat_s = run(fn, cfg, generic=False)
    gen, _, sat_g = run(fn, cfg, generic=True)
    assert sat_s and sat_g
    assert torch.equal(spec.hl, gen.hl)


@gpu
@pytest.mark.parametrize("cfg", TILES)
@torch.no_grad()
def test_winograd_products_equal_generic_body(f16x3, monkeypatch, cfg):
    """The grouped dense products of a Winograd F(4x4, 3x3) convolution (fp32 Y, no bias: PP_EPI_C_PLAIN)."""
    from picopose_amd import ops

    monkeypatch.setattr(ops, "WINOGRAD4", True)
    B, hw, cin, cout = 8, 32, 64, 256                      # (N = 256: a pinned 256x256 tile is not narrowed to 256x128)
    g = torch.Generator().manual_seed(cfg)
    x = torch.randn(B, hw, hw, cin, generator=g).cuda()
    wp = ops.pack_conv_weight((torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).cuda())
    bias = torch.randn(cout, generator=g).cuda()
    xs = ops.split_image(x)
    fn = lambda: ops.conv2d(xs, wp, bias, 3, pad=1, act="relu", wino=True)  # noqa: E731
    spec, rs, _ = run(fn, cfg, generic=False)
    gen, rg, _ = run(fn, cfg, generic=True)
    assert rs and all(r["cfg"] == cfg and r["amode"] == 0 for r in rs), rs
    assert torch.equal(spec, gen)
