"""The Winograd transforms (csrc/pp_winograd.hip) and the narrow predict layers (conv_narrow_kernel) against the float64 element-wise
bounds of tests/wino_bounds.py (derivation there; tests/test_wino_bounds_cpu.py shows that they discriminate).  Stage tests call the
transform kernels on their own through the C ABI as ops.py does; the end-to-end tests run ops.conv2d / conv2d_wino_pair on every case and
prove the route from the engine's launch records (16 resp. 36 products, one grouped launch where the tile count allows it)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_bounds as eb  # noqa: E402
import wino_bounds as wb  # noqa: E402

gpu = pytest.mark.gpu
ACT = {None: 0, "relu": 1, "leaky01": 3}
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _worst_summary():
    before = dict(eb.WORST)
    yield
    for key, (r, name) in sorted(eb.WORST.items()):
        if key.startswith("wino ") and before.get(key) != (r, name):
            print(f"[bound] worst |err|/bound of {key}: {r:.3g} ({name})", flush=True)


@pytest.fixture
def env(monkeypatch):
    """ops in a known state: Winograd on at every size, the saturation word registered and clear"""
    from picopose_amd import _lib, ops

    monkeypatch.setattr(ops, "WINOGRAD", True)
    monkeypatch.setattr(ops, "WINOGRAD4", True)
    monkeypatch.setattr(ops, "WINOGRAD_MIN_PIXELS", 0)
    monkeypatch.delenv("PP_GEMM_FORCE_CFG", raising=False)
    for k, v in ACT.items():
        assert ops.ACT[k] == v
    ops.saturation_raised()
    yield ops, _lib.lib(), _lib
    ops.drop_split_cache()
    ops.saturation_raised()


def launched(fn):
    """fn() -> (result, the engine's launch records of the call: M, N, K, conv kernel size, configuration, kind, A-delivery mode), as
    tests/test_engine_bounds_gpu.py reads them.  A first, unrecorded call lets the engine choose its configuration for new shapes."""
    from picopose_amd import _lib

    L, cap = _lib.lib(), 64
    fn()
    _lib.check(L.pp_prof_gemm_enable(cap), "pp_prof_gemm_enable")
    try:
        out = fn()
        torch.cuda.synchronize()
        shape, ms = (ctypes.c_int * (8 * cap))(), (ctypes.c_float * cap)()
        fl, by, cnt = (ctypes.c_double * cap)(), (ctypes.c_double * cap)(), ctypes.c_int()
        _lib.check(L.pp_prof_gemm_records2(cap, shape, ms, fl, by, ctypes.byref(cnt)), "pp_prof_gemm_records2")
    finally:
        _lib.check(L.pp_prof_gemm_enable(0), "pp_prof_gemm_enable")
    keys = ("M", "N", "K", "k", "cfg", "kind", "amode")
    return out, [dict(zip(keys, (shape[8 * i + j] for j in range(7)))) for i in range(cnt.value)]


def _ref(op, c):
    key = wb.case_name(op, c)
    if key not in _REF:
        inp = wb.inputs(op, c)
        _REF[key] = (inp, wb.reference(op, c, inp))
    return _REF[key]


def _check(op, c, got, ref, bound, what=""):
    eb.check(wb.case_name(op, c) + what, got, ref, bound, "wino " + op)


def _vals(hl, C, scale):
    """the values (hi + lo) / scale of an hl operand buffer (rows, 2 C)"""
    return hl.view(hl.shape[0], C // 8, 2, 8).double().sum(2).reshape(hl.shape[0], C) / scale


def _operand(ops, x, wide=0):
    """the hl operand image of x (already 22-bit values), optionally as columns 8 .. 8 + C of an operand `wide` channels wider -> (Split, col0)"""
    B, H, W, C = x.shape
    src = x
    if wide:
        src = torch.full((B, H, W, C + wide), 3.0)
        src[..., 8:8 + C] = x
    xs = ops.split_image(src.cuda())
    assert isinstance(xs, ops.Split) and xs.terms == 2
    col0 = 8 if wide else 0
    assert torch.equal(_vals(xs.hl, C + wide, 4.0)[:, col0:col0 + C].cpu(), x.double().reshape(-1, C)), "the operand holds other values than the case's"
    return xs, col0


def _strided(x, ld, extra):
    """x (B, H, W, C) on the device as channels 4 .. 4 + C of rows `ld` wide, images `extra` floats apart; the rest NaN (never read)"""
    B, H, W, C = x.shape
    buf = torch.full((B, H * W * ld + extra), float("nan"), device="cuda")
    v = buf[:, :H * W * ld].view(B, H, W, ld)[..., 4:4 + C]
    v.copy_(x)
    return v


# ------------------------------------------------------------------------------------------------------------------ stage tests
@gpu
@torch.no_grad()
def test_input_transforms(env, monkeypatch):
    ops, L, _lib = env
    for i, c in enumerate(wb.CASES["in2"]):
        inp, (ref, bound) = _ref("in2", c)
        B, H, W, C = inp["x"].shape
        x = _strided(inp["x"], C + 8, 64) if i % 2 else inp["x"].cuda()        # a channel slice with a free batch stride | contiguous
        U = torch.full((16, B * (H // 2) * (W // 2), C), float("nan"), device="cuda")
        _lib.check(L.pp_winograd_input_f32(x.data_ptr(), x.stride(2), x.stride(0), B, H, W, C, int(c["relu"]), U.data_ptr(), _lib.stream_ptr()), "in2")
        _check("in2", c, U, ref, bound)
        assert not bool(U.cpu()[bound == 0].any())                              # a zero window, a dead input: exactly 0
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    for i, c in enumerate(wb.CASES["in4"]):
        inp, (ref, bound) = _ref("in4", c)
        B, H, W, C = inp["x"].shape
        xs, col0 = _operand(ops, inp["x"], wide=16 if i % 2 else 0)              # a channel slice of a wider operand | the operand itself
        P = B * (H // 4) * (W // 4)
        Pp = ops._wino4_rows(P)
        U = torch.zeros(36 * Pp, 2 * C, dtype=torch.float16, device="cuda")
        _lib.check(L.pp_winograd4_input_hl(xs.col_ptr(col0), xs.shape[1], H * W * xs.shape[1], B, H, W, C, int(c["relu"]), U.data_ptr(), Pp,
                                           _lib.stream_ptr()), "in4")
        got = (_vals(U, C, 1.0 / 16.0)).view(36, Pp, C)
        _check("in4", c, got[:, :P], ref, bound)
        assert not bool(got[:, :P].cpu()[bound == 0].any())
        assert not bool(U.view(36, Pp, 2 * C)[:, P:].any()), "pad rows written"
        assert not ops.saturation_raised()


@gpu
@torch.no_grad()
def test_weight_transforms(env):
    ops, L, _lib = env
    for fam, fn in ((2, lambda wp, ci: ops.winograd_weight(wp, ci)), (4, lambda wp, ci: ops.winograd4_weight(wp, ci)[0])):
        for c in wb.CASES[f"wt{fam}"]:
            inp, (ref, bound) = _ref(f"wt{fam}", c)
            wp = ops.pack_conv_weight(inp["w"].cuda())
            _check(f"wt{fam}", c, fn(wp, c["Cin"]).view(ref.shape), ref, bound)


def _out_args(inp, c, wide):
    """device forms of the output transform's operands; `wide`: out and the residuals as channels 4 .. 4 + C of rows C + 8 wide"""
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    mk = (lambda t: _strided(t, C + 8, 0)) if wide else (lambda t: t.cuda())
    out = mk(torch.full((B, H, W, C), float("nan")))
    r = [mk(inp[k]) if k in inp else None for k in ("r1", "r2")]
    bias = inp["bias"].cuda() if "bias" in inp else None
    return out, r, bias


def _untouched(out):
    """the neighbours of a channel-slice output (made by _strided: NaN everywhere else) are still NaN"""
    B, H, W, C = out.shape
    ld = out.stride(2)
    base = torch.as_strided(out, (B, H, W, ld), (out.stride(0), out.stride(1), ld, 1), out.storage_offset() - 4)
    return bool(torch.isnan(base[..., :4]).all()) and bool(torch.isnan(base[..., 4 + C:]).all())


@gpu
@torch.no_grad()
def test_output_transforms(env, monkeypatch):
    ops, L, _lib = env
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    for i, c in enumerate(wb.CASES["out2"]):
        inp, (ref, bound) = _ref("out2", c)
        B, H, W, C = c["B"], c["H"], c["W"], c["C"]
        wide = i % 2 == 1 and C % 4 == 0
        out, r, bias = _out_args(inp, c, wide)
        _lib.check(L.pp_winograd_output_f32(inp["Y"].cuda().data_ptr(), B, H, W, C, p(bias), ACT[c["act"]], p(r[0]), p(r[1]), out.data_ptr(),
                                            out.stride(2), _lib.stream_ptr()), "out2")
        _check("out2", c, out, ref, bound)
        assert not wide or _untouched(out)
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    for i, c in enumerate(wb.CASES["out4"]):
        inp, (ref, bound) = _ref("out4", c)
        B, H, W, C = c["B"], c["H"], c["W"], c["C"]
        P = B * (H // 4) * (W // 4)
        Pp = ops._wino4_rows(P)
        # Y as columns 4 .. 4 + C of a wider product (two layers fused along N), pad rows NaN (never read)
        ycol, ldy = (4, C + 8) if i % 2 else (0, C)
        Y = torch.full((36, Pp, ldy), float("nan"), device="cuda")
        Y[:, :P, ycol:ycol + C] = inp["Y"].cuda()
        yp = Y.data_ptr() + 4 * ycol
        wide = i % 3 == 1 and not c["hl"]
        out, r, bias = _out_args(inp, c, wide)
        hl = torch.zeros(B * H * W, 2 * C, dtype=torch.float16, device="cuda") if c["hl"] else None
        _lib.check(L.pp_winograd4_output(yp, ldy, B, H, W, C, p(bias), ACT[c["act"]], p(r[0]), p(r[1]), None if c["hl"] else out.data_ptr(),
                                         0 if c["hl"] else out.stride(2), p(hl), C, int(bool(c.get("c_relu"))), Pp, _lib.stream_ptr()), "out4")
        got = _vals(hl, C, 4.0).view(B, H, W, C) if c["hl"] else out
        _check("out4", c, got, ref, bound)
        assert not wide or _untouched(out)
        assert not ops.saturation_raised()


@gpu
@torch.no_grad()
def test_chained_transforms(env, monkeypatch):
    """U1 of the chain kernels against in(out(Y)) in float64 under the composed bound, and bit for bit against the two separate kernels, on
    one tile row (the ring never fills), five (it wraps), H != W, and the three widths"""
    ops, L, _lib = env
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    for c in wb.CASES["chain2"]:
        inp, (ref, bound) = _ref("chain2", c)
        B, H, W, C = c["B"], c["H"], c["W"], c["C"]
        P = B * (H // 2) * (W // 2)
        Y = inp["Y"].cuda()
        bias = inp["bias"].cuda() if "bias" in inp else None
        U1 = torch.full((16, P, C), float("nan"), device="cuda")
        U2 = torch.full((16, P, C), float("nan"), device="cuda")
        h = torch.full((B, H, W, C), float("nan"), device="cuda")
        _lib.check(L.pp_winograd_chain_f32(Y.data_ptr(), B, H, W, C, p(bias), ACT[c["act"]], int(c["c_relu"]), U1.data_ptr(), _lib.stream_ptr()), "chain2")
        _lib.check(L.pp_winograd_output_f32(Y.data_ptr(), B, H, W, C, p(bias), ACT[c["act"]], None, None, h.data_ptr(), C, _lib.stream_ptr()), "out2")
        _lib.check(L.pp_winograd_input_f32(h.data_ptr(), C, H * W * C, B, H, W, C, int(c["c_relu"]), U2.data_ptr(), _lib.stream_ptr()), "in2")
        assert torch.equal(U1, U2), wb.case_name("chain2", c)
        _check("chain2", c, U1, ref, bound)
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    for c in wb.CASES["chain4"]:
        inp, (ref, bound) = _ref("chain4", c)
        B, H, W, C = c["B"], c["H"], c["W"], c["C"]
        P = B * (H // 4) * (W // 4)
        Pp = ops._wino4_rows(P)
        Y = torch.full((36, Pp, C), float("nan"), device="cuda")
        Y[:, :P] = inp["Y"].cuda()
        bias = inp["bias"].cuda() if "bias" in inp else None
        U1 = torch.zeros(36 * Pp, 2 * C, dtype=torch.float16, device="cuda")
        U2 = torch.zeros(36 * Pp, 2 * C, dtype=torch.float16, device="cuda")
        h = torch.zeros(B * H * W, 2 * C, dtype=torch.float16, device="cuda")
        _lib.check(L.pp_winograd4_chain(Y.data_ptr(), C, B, H, W, C, p(bias), ACT[c["act"]], int(c["c_relu"]), U1.data_ptr(), Pp, _lib.stream_ptr()), "chain4")
        _lib.check(L.pp_winograd4_output(Y.data_ptr(), C, B, H, W, C, p(bias), ACT[c["act"]], None, None, None, 0, h.data_ptr(), C, int(c["c_relu"]), Pp,
                                         _lib.stream_ptr()), "out4")
        _lib.check(L.pp_winograd4_input_hl(h.data_ptr(), C, H * W * C, B, H, W, C, 0, U2.data_ptr(), Pp, _lib.stream_ptr()), "in4")
        assert torch.equal(U1, U2), wb.case_name("chain4", c)
        _check("chain4", c, _vals(U1, C, 1.0 / 16.0).view(36, Pp, C)[:, :P], ref, bound)
        assert not bool(U1.view(36, Pp, 2 * C)[:, P:].any()), "pad rows written"
        assert not ops.saturation_raised()


# ------------------------------------------------------------------------------------------------------------------ end to end
def _products_ran(recs, n, P, rows, cin, cout, kind):
    """the engine's launch records show the n Winograd products (K = Cin, N = Cout, dense): ONE grouped launch over n x rows rows where a
    row tile lies inside one product (rows % 256 == 0), else n launches of P rows"""
    assert all(r["k"] == 0 and r["K"] == cin and r["N"] == cout and r["kind"] == kind for r in recs), recs
    if rows % 256 == 0:
        assert [r["M"] for r in recs] == [n * rows], (n, rows, recs)
    else:
        assert [r["M"] for r in recs] == [P] * n, (n, P, recs)


@gpu
@torch.no_grad()
def test_convolution_f2x2_end_to_end(env, monkeypatch):
    ops, L, _lib = env
    monkeypatch.setattr(ops, "PRECISION", "f32")
    for i, c in enumerate(wb.CASES["conv_w2"]):
        inp, (ref, bound) = _ref("conv_w2", c)
        B, H, W, Ci, Co = c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
        x = _strided(inp["x"], Ci + 8, 64 if i % 4 == 1 else 0) if i % 2 else inp["x"].cuda()
        wp = ops.pack_conv_weight(inp["w"].cuda())
        wide = i % 3 == 2 and Co % 4 == 0
        out, r, bias = _out_args(inp, dict(c, C=Co), wide)
        fn = lambda: ops.conv2d(x, wp, bias, 3, pad=1, act=c["act"], relu_in=c["relu_in"], residual=r[0], residual2=r[1], out=out if wide else None,   # noqa: E731
                                cin=Ci)
        got, recs = launched(fn)
        P = B * (H // 2) * (W // 2)
        _products_ran(recs, 16, P, P, Ci, Co, kind=1)
        _check("conv_w2", c, got, ref, bound)
        assert not wide or _untouched(out)
        if c["kind"] == "dead":      # nothing passes the input ReLU: act(bias) + residuals in the epilogue's fp32 order, exactly
            want = wb._act(inp["bias"] if "bias" in inp else torch.zeros(Co), c["act"]).expand(B, H, W, -1)
            for k in ("r1", "r2"):
                want = want + inp[k] if k in inp else want
            assert torch.equal(got.cpu(), want), wb.case_name("conv_w2", c)


def _as_maps(ops, res, c, Co):
    """the results of an F(4x4) layer as float64 maps in the order of the reference"""
    B, H, W = c["B"], c["H"], c["W"]
    if isinstance(res, ops.Split):
        return _vals(res.hl, Co, 4.0).view(B, H, W, Co)
    if c.get("also"):
        return (res, _vals(res._hl_relu.hl, Co, 4.0).view(B, H, W, Co))
    return res


@gpu
@torch.no_grad()
def test_convolution_f4x4_end_to_end(env, monkeypatch):
    ops, L, _lib = env
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    monkeypatch.setattr(ops, "CHECK_SATURATION", True)
    for i, c in enumerate(wb.CASES["conv_w4"]):
        inp, (ref, bound) = _ref("conv_w4", c)
        B, H, W, Ci, Co = c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
        xs, col0 = _operand(ops, inp["x"], wide=16 if i % 2 else 0)
        wp = ops.pack_conv_weight(inp["w"].cuda())
        wide = i % 3 == 2 and not c["hl"] and not c.get("also")
        out, r, bias = _out_args(inp, dict(c, C=Co), wide)
        kw = dict(in_cols=(col0, Ci)) if col0 else {}
        fn = lambda: ops.conv2d(xs, wp, bias, 3, pad=1, act=c["act"], residual=r[0], residual2=r[1], out=out if wide else None, out_split=c["hl"],   # noqa: E731
                                split_relu=bool(c.get("c_relu")), also_split=c.get("also"), wino=True, **kw)
        res, recs = launched(fn)
        P = B * (H // 4) * (W // 4)
        _products_ran(recs, 36, P, ops._wino4_rows(P), Ci, Co, kind=0)
        got = _as_maps(ops, res, c, Co)
        if isinstance(got, tuple):
            for g_, r_, b_, nm in zip(got, ref, bound, (" map", " operand")):
                _check("conv_w4", c, g_, r_, b_, nm)
        else:
            _check("conv_w4", c, got, ref, bound)
        assert not wide or _untouched(out)
        assert not ops.saturation_raised()
    # two layers on one input as ONE product per frequency, Ca != Cb: the second layer reads Y at a column offset
    for c in wb.CASES["pair4"]:
        inp, (ref, bound) = _ref("pair4", c)
        xs, _ = _operand(ops, inp["x"])
        la = (ops.pack_conv_weight(inp["w"].cuda()), inp["bias"].cuda())
        lb = (ops.pack_conv_weight(inp["wb"].cuda()), inp["biasb"].cuda())
        fn = lambda nxt=False: ops.conv2d_wino_pair(xs, la, lb, act=c["act"], out_split=True, split_relu=c["c_relu"], wino_next=nxt)   # noqa: E731
        (ra, rb), recs = launched(fn)
        P = c["B"] * (c["H"] // 4) * (c["W"] // 4)
        _products_ran(recs, 36, P, ops._wino4_rows(P), c["Cin"], c["Ca"] + c["Cb"], kind=0)
        for res, co, r_, b_, nm in ((ra, c["Ca"], ref[0], bound[0], " a"), (rb, c["Cb"], ref[1], bound[1], " b")):
            assert isinstance(res, ops.Split)
            _check("pair4", c, _vals(res.hl, co, 4.0).view(r_.shape), r_, b_, nm)
        na, nb = fn(True)          # (these widths do not chain: the same operands come back)
        assert torch.equal(na.hl, ra.hl) and torch.equal(nb.hl, rb.hl)


@gpu
@torch.no_grad()
def test_operand_range_edge_of_f4x4(env, monkeypatch):
    """U = B^T d B / 16 leaves the fp16 range at |d| >= 10 480 although the source operand holds up to 16 376.  d = a s_i s_j with
    s = (+, 0, -, 0, +, 0) over the 6x6 window of an INTERIOR tile (a one-tile image has the window's outer ring in the zero padding) gives
    |U_00| = 100 a: at a = 10 000 (U / 16 = 62 500) the saturation word stays 0 and the result is inside the bound; at a = 11 000 (68 750) the
    word is raised — the flagged result holds +-inf / NaN terms and is WRONG, nothing else about it is asserted.  The same for the operand
    output of pp_winograd4_output around |h| = 16 376 (4 h = 65 504)."""
    ops, L, _lib = env
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    s = torch.tensor([1.0, 0.0, -1.0, 0.0, 1.0, 0.0])
    c = dict(B=1, H=12, W=12, C=8, kind="edge", relu=False)
    for a, flagged in ((10000.0, False), (11000.0, True)):
        x = torch.zeros(1, 12, 12, 8)
        x[0, 3:9, 3:9, :] = (a * s.view(6, 1) * s.view(1, 6)).unsqueeze(-1)
        xs, _ = _operand(ops, x)
        assert not ops.saturation_raised()
        U = ops._winograd4_input(xs.hl.data_ptr(), 8, 1, 12, 12, 8, xs.device)
        assert ops.saturation_raised() == flagged
        if not flagged:
            ref, bound = wb.reference("in4", c, dict(x=x))
            assert float(ref.abs().max()) == 100 * a
            _check("in4", dict(c, a=a), _vals(U.hl, 8, 1.0 / 16.0).view(36, 256, 8)[:, :9], ref, bound)
    co = dict(B=1, H=4, W=4, C=8, kind="edge", bias=False, act=None, nres=0, hl=True, c_relu=False)
    for v, flagged in ((16000.0, False), (-16000.0, False), (16380.0, True)):
        Y = torch.zeros(36, 256, 8)
        Y[0, 0, :] = v                                                          # A^T Y A of frequency (0, 0) alone: pixel (0, 0) of the tile
        hl = torch.zeros(16, 16, dtype=torch.float16, device="cuda")
        _lib.check(L.pp_winograd4_output(Y.cuda().data_ptr(), 8, 1, 4, 4, 8, None, 0, None, None, None, 0, hl.data_ptr(), 8, 0, 256, _lib.stream_ptr()), "out4")
        assert ops.saturation_raised() == flagged
        if not flagged:
            ref, bound = wb.reference("out4", co, dict(Y=Y[:, :1]))
            assert float(ref[0, 0, 0, 0]) == v
            _check("out4", dict(co, v=v), _vals(hl, 8, 4.0).view(1, 4, 4, 8), ref, bound)


@gpu
@pytest.mark.parametrize("mode", ["f32", "f16x3", "f16"])
@torch.no_grad()
def test_narrow_predict_layers(env, monkeypatch, mode):
    """pp_conv_narrow_f32 on the fp32 map (f32) and pp_conv_narrow_hl on the operand (f16x3) against `narrow`.  The f16 mode has no narrow
    kernel (its operand has one term): the layers run on the engine there and are held to the engine's own f16 bound."""
    ops, L, _lib = env
    monkeypatch.setattr(ops, "PRECISION", mode)
    for c in wb.CASES["narrow"]:
        if c["hl"] != (mode != "f32"):
            continue
        inp, (ref, bound) = _ref("narrow", c)
        x = inp["x"].cuda()
        xs = x if mode == "f32" else ops.split_image(x)
        wp = ops.pack_conv_weight(inp["w"].cuda())
        res = inp["r1"].cuda() if "r1" in inp else None
        got, recs = launched(lambda: ops.conv2d(xs, wp, inp["bias"].cuda(), c["k"], pad=c["k"] // 2, residual=res))
        if mode == "f16":
            assert len(recs) == 1
            ref, bound = eb.reference("conv2d", inp["x"].permute(0, 3, 1, 2), inp["w"], "f16", bias=inp["bias"], padding=c["k"] // 2,
                                      residual=None if res is None else inp["r1"].permute(0, 3, 1, 2), device="cpu")
            ref, bound = ref.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1)
        else:
            assert recs == [], "the narrow layer went to the engine"
        _check("narrow " + mode, c, got, ref, bound)


# ------------------------------------------------------------------------------------------------------------------ contracts
@gpu
@torch.no_grad()
def test_shared_and_chained_winograd_inputs_carry_their_relu(env, monkeypatch):
    """A shared WinoInput made with the input ReLU must be asked for it by every consumer, and one made without must not be; a chained
    one (conv2d(..., wino_next="relu")) already holds its single consumer's ReLU and is taken either way.  F(4x4): wino_next="relu" folds
    the consumer's ReLU into the operand exactly as split_relu does."""
    ops, L, _lib = env
    monkeypatch.setattr(ops, "PRECISION", "f32")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 16, 32, generator=g).cuda()
    w1 = ops.pack_conv_weight((torch.randn(32, 32, 3, 3, generator=g) / 17).cuda())
    w2 = ops.pack_conv_weight((torch.randn(32, 32, 3, 3, generator=g) / 17).cuda())
    sh = ops.winograd_shared(x, relu=True)
    assert isinstance(sh, ops.WinoInput) and sh.relu and not sh.chained
    assert torch.equal(ops.conv2d(sh, w1, None, 3, pad=1, relu_in=True), ops.conv2d(x, w1, None, 3, pad=1, relu_in=True))
    with pytest.raises(AssertionError):
        ops.conv2d(sh, w1, None, 3, pad=1)                       # made with a ReLU this layer does not ask for
    with pytest.raises(AssertionError):
        ops.conv2d(ops.winograd_shared(x), w1, None, 3, pad=1, relu_in=True)
    ch = ops.conv2d(x, w1, None, 3, pad=1, wino_next="relu")
    assert isinstance(ch, ops.WinoInput) and ch.relu and ch.chained
    want = ops.conv2d(ops.conv2d(x, w1, None, 3, pad=1), w2, None, 3, pad=1, relu_in=True)
    assert torch.equal(ops.conv2d(ch, w2, None, 3, pad=1), want) and torch.equal(ops.conv2d(ch, w2, None, 3, pad=1, relu_in=True), want)
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    xs = ops.split_image((x * 3).contiguous())
    for shape_chains, widths in ((False, ()), (True, (16, 32, 64))):
        monkeypatch.setattr(ops, "WINO4_CHAIN_WIDTHS", widths)
        a = ops.conv2d(xs, w1, None, 3, pad=1, out_split=True, wino=True, wino_next="relu")
        b = ops.conv2d(xs, w1, None, 3, pad=1, out_split=True, split_relu=True, wino=True, wino_next=True)
        plain = ops.conv2d(xs, w1, None, 3, pad=1, out_split=True, wino=True, wino_next=True)
        assert isinstance(a, ops.WinoInput4) == shape_chains
        ha, hb, hp = ((t.U.hl, ) if shape_chains else (t.hl, ) for t in (a, b, plain))
        assert torch.equal(ha[0], hb[0]) and not torch.equal(ha[0], hp[0])
