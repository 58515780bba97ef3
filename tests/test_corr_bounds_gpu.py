"""The correlation lookup, its adjoint and the loss kernels on the GPU against the float64 references and element-wise bounds of tests/corr_bounds.py: every
arithmetic mode of pp_corr_lookup_nhwc_ex on the tiled and the lane-per-position kernel, the operand-input branch (ring and register-staged,
bit-equal to the fp32-input f16x3 result), the pad channels, non-finite flows, pooled axes of size 1; the per-pixel and the patch form of the
adjoint, atomic and deterministic; gather + normalise, the diagonal cross entropy, the flow / certainty loss sums, their adjoints and the
ordered row scatter.  The references are computed in this process on the CPU from torch's float64 ops."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corr_bounds as cb  # noqa: E402

gpu = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios_summary():
    """after the last test of this file that ran: the worst |err| / bound per operation and mode (the figures of DESIGN.md)"""
    yield
    for key, (worst, where) in sorted(cb.eb.WORST.items()):
        if key.split()[0] in ("corr", "corr_bwd") + cb.LOSS_OPS:
            print(f"[worst] {key}: {worst:.3g} at {where}", flush=True)


def _ids(op):
    return [f"{i}-{c['H']}x{c['W']}-L{c['L']}-r{c['r']}-C{c['C']}-{c['kind']}" for i, c in enumerate(cb.CASES[op])]


def _operands(ops, f1, f2):
    B, H, W, C = f1.shape
    wide = ops.Split.empty(B * H * W, 96 if C <= 64 else C + 32, f1.device)                     # f1 as columns 32.. of a wider operand
    wide.hl.zero_()
    ops.split_activation(f1, B, H * W, C, H * W * C, C, into=(wide, 32))
    f2s = ops.Split(ops.split_activation(f2, f2.shape[0], H * W, C, H * W * C, C))
    return dict(f1_hl=(wide, 32), f2_hl=f2s)


@gpu
@pytest.mark.parametrize("c", cb.CASES["corr"], ids=_ids("corr"))
def test_lookup_stays_inside_the_float64_bound(monkeypatch, c):
    from picopose_amd import ops

    name = cb.case_name("corr", c)
    inp = cb.inputs("corr", c)
    f1, f2, flow = (inp[k].cuda() for k in ("f1", "f2", "flow"))
    H, W, C, L, r = c["H"], c["W"], c["C"], c["L"], c["r"]
    n = L * (2 * r + 1) ** 2
    tiled = H % 8 == 0 and W % 8 == 0 and C % 32 == 0
    bounds = {m: cb.reference("corr", c, inp, m) for m in (cb.MODES if tiled else ("f32",))}

    def run(mode, pad, **kw):
        with ops.precision_scope(mode):
            out = ops.corr_lookup(kw.pop("f1", f1), f2, flow, L, r, c_pad=pad, **kw)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (c["B"], H, W, max(pad or n, n))
        assert not bool(out[..., n:].any()), f"{name}: pad channels"
        return out

    for pad in (None, -(-n // 8) * 8):
        # the lane-per-position kernel: fp32 products in every mode (finer than f16 asks for): held to the f32 bound
        monkeypatch.setenv("PP_CORR_TILED", "0")
        for mode in cb.MODES:
            out = run(mode, pad)
            cb.check(f"{name} lane/{mode} pad={pad}", out[..., :n], *bounds["f32"], mode="corr lane")
        monkeypatch.delenv("PP_CORR_TILED")
        if not tiled:
            continue
        for mode in cb.MODES:
            out = run(mode, pad)
            cb.check(f"{name} tiled/{mode} pad={pad}", out[..., :n], *bounds[mode], mode="corr tiled " + mode)
            if mode == "f16x3":
                x3 = out
        hl = _operands(ops, f1, f2)
        assert ops.corr_takes_operands(hl["f1_hl"], hl["f2_hl"], H, W, C)
        for ring in ("1", "0"):
            monkeypatch.setenv("PP_CORR_RING", ring)
            got = run("f16x3", pad, f1=None, **hl)
            assert torch.equal(got, x3), f"{name}: operand input (PP_CORR_RING={ring}) differs from the fp32-input f16x3 result"
        monkeypatch.delenv("PP_CORR_RING")


def _adjoint(ag, f1, f2, flow, dout, L, r):
    ctx = types.SimpleNamespace(saved_tensors=(f1, f2, flow), cfg=(L, r))
    df1, df2, dflow = ag._CorrLookup.backward(ctx, dout)[:3]
    torch.cuda.synchronize()
    return df1, df2, dflow


@gpu
@pytest.mark.parametrize("c", cb.CASES["corr_bwd"], ids=_ids("corr_bwd"))
def test_lookup_adjoint_stays_inside_the_float64_bound(monkeypatch, c):
    from picopose_amd import autograd as ag

    name = cb.case_name("corr_bwd", c)
    inp = cb.inputs("corr_bwd", c)
    f1, f2, flow, dout = (inp[k].cuda().contiguous() for k in ("f1", "f2", "flow", "dout"))
    H, W, C, L, r = c["H"], c["W"], c["C"], c["L"], c["r"]
    patch = H % 4 == 0 and W % 4 == 0 and C % 128 == 0
    bad = cb._bad(inp["flow"])
    for det in (False, True):
        monkeypatch.setattr(ag, "DETERMINISTIC", det)
        ref, bound = cb.reference("corr_bwd", c, inp, det=det)
        for per_pixel in ((True, False) if patch else (True,)):
            if per_pixel:
                monkeypatch.setenv("PP_CORR_SCATTER_PER_PIXEL", "1")
            else:
                monkeypatch.delenv("PP_CORR_SCATTER_PER_PIXEL", raising=False)
            got = _adjoint(ag, f1, f2, flow, dout, L, r)
            tag = f"{name} {'per-pixel' if per_pixel else 'patch'}{' det' if det else ''}"
            key = "corr_bwd" + (" det" if det else "")
            for what, g, rf, b in zip(("df1", "df2", "dflow"), got, ref, bound):
                cb.check(f"{tag} {what}", g, rf, b, mode=f"{key} {what}")
            assert not bool(got[0].cpu()[bad].any()) and not bool(got[2].cpu()[bad].any()), f"{tag}: a non-finite flow hands a gradient on"
            if det:
                again = _adjoint(ag, f1, f2, flow, dout, L, r)
                assert all(torch.equal(a, b) for a, b in zip(got, again)), f"{tag}: two runs differ"
        monkeypatch.delenv("PP_CORR_SCATTER_PER_PIXEL", raising=False)


def _lids(op):
    return [",".join(f"{k}={v}" for k, v in c.items()) for c in cb.CASES[op]]


def _lib():
    from picopose_amd import _lib as L

    return L, L.lib(), L.stream_ptr()


@gpu
@pytest.mark.parametrize("c", cb.CASES["gather_normalize"], ids=_lids("gather_normalize"))
def test_gather_normalize_rows(c):
    M, L, st = _lib()
    inp = cb.inputs("gather_normalize", c)
    ref, bound = cb.reference("gather_normalize", c, inp)
    src, index = inp["src"].cuda(), inp["index"].cuda()
    out = torch.empty(c["n"], c["C"], dtype=torch.float32, device="cuda")
    M.check(L.pp_gather_normalize_rows(src.data_ptr(), src.stride(0), index.data_ptr(), c["n"], c["C"], 1e-12, out.data_ptr(), st), "pp_gather_normalize_rows")
    cb.check(cb.case_name("gather_normalize", c), out, ref, bound, mode="gather_normalize")
    assert not bool(out[0].any())                                                                        # the zero row


@gpu
@pytest.mark.parametrize("c", cb.CASES["normalize_bwd_indexed"], ids=_lids("normalize_bwd_indexed"))
def test_normalize_rows_backward_with_an_index(c):
    M, L, st = _lib()
    inp = cb.inputs("normalize_bwd_indexed", c)
    ref, bound = cb.reference("normalize_bwd_indexed", c, inp)
    src, index, dq = inp["src"].cuda(), inp["index"].cuda(), inp["dq"].cuda()
    dx = torch.empty(c["n"], c["C"], dtype=torch.float32, device="cuda")
    M.check(L.pp_normalize_rows_backward(src.data_ptr(), src.stride(0), index.data_ptr(), dq.data_ptr(), c["n"], c["C"], 1e-12, dx.data_ptr(), st),
            "pp_normalize_rows_backward")
    cb.check(cb.case_name("normalize_bwd_indexed", c), dx, ref, bound, mode="normalize_bwd_indexed")


@gpu
@pytest.mark.parametrize("c", cb.CASES["xent_diag"], ids=_lids("xent_diag"))
def test_xent_diag_rows_and_backward(c):
    M, L, st = _lib()
    n, ld, s = c["n"], c["ld"], c["scale"]
    inp = cb.inputs("xent_diag", c)
    ref, bound = cb.reference("xent_diag", c, inp)
    lg = inp["L"].cuda()
    rows = torch.empty(n, dtype=torch.float32, device="cuda")
    M.check(L.pp_xent_diag_rows(lg.data_ptr(), n, ld, s, rows.data_ptr(), st), "pp_xent_diag_rows")
    cb.check(cb.case_name("xent_diag", c), rows, ref, bound, mode="xent_diag")
    if n == 1:
        assert float(rows[0]) == 0.0
    cbw = dict(c)
    if cbw in cb.CASES["xent_diag_bwd"]:
        inp = cb.inputs("xent_diag_bwd", cbw)
        ref, bound = cb.reference("xent_diag_bwd", cbw, inp)
        lg, up = inp["L"].cuda(), inp["up"].cuda()
        dl = torch.empty(n, n, dtype=torch.float32, device="cuda")
        M.check(L.pp_xent_diag_backward(lg.data_ptr(), n, ld, s, up.data_ptr(), dl.data_ptr(), st), "pp_xent_diag_backward")
        cb.check(cb.case_name("xent_diag_bwd", cbw), dl, ref, bound, mode="xent_diag_bwd")


@gpu
@pytest.mark.parametrize("c", cb.CASES["flow_loss"], ids=_lids("flow_loss"))
def test_flow_loss_sums_and_backward(c):
    from picopose_amd import autograd as ag

    M, L, st = _lib()
    B, H, W = c["B"], c["H"], c["W"]
    mf = cb.f32(c["max_flow"])
    inp = cb.inputs("flow_loss_bwd", c)
    ref, bound = cb.reference("flow_loss", c, inp)
    fl, ce, tp, gf, gc = (inp[k].cuda() for k in ("flow", "cert", "pts", "gf", "gc"))
    part = torch.empty(L.pp_flow_loss_blocks(), 3, dtype=torch.float64, device="cuda")
    M.check(L.pp_flow_loss_sums(fl.data_ptr(), ce.data_ptr(), tp.data_ptr(), B, H, W, mf, part.data_ptr(), st), "pp_flow_loss_sums")
    cb.check(cb.case_name("flow_loss", c), part.sum(0), ref, bound, mode="flow_loss")
    lf, lc = ag.flow_level_losses(fl, ce, tp, max_flow=mf)
    assert bool(torch.isfinite(lf)) and bool(torch.isfinite(lc))
    if float(ref[2]) == 0.0:
        assert float(lf) == 0.0                                                                          # l1 / (0 + eps): 0, not NaN
    (rfl, rce), (bfl, bce) = cb.reference("flow_loss_bwd", c, inp)
    dfl, dce = torch.empty_like(fl), torch.empty_like(ce)
    M.check(L.pp_flow_loss_backward(fl.data_ptr(), ce.data_ptr(), tp.data_ptr(), B, H, W, mf, gf.data_ptr(), gc.data_ptr(), dfl.data_ptr(), dce.data_ptr(), st),
            "pp_flow_loss_backward")
    # dflow: exactly +-kf or 0 (bound 0) outside the exempt positions
    cb.check(cb.case_name("flow_loss_bwd", c) + " dflow", dfl.double(), rfl.float().double(), bfl, mode="flow_loss_bwd dflow")
    cb.check(cb.case_name("flow_loss_bwd", c) + " dcert", dce, rce, bce, mode="flow_loss_bwd dcert")


@gpu
@pytest.mark.parametrize("c", cb.CASES["scatter_add_rows"], ids=_lids("scatter_add_rows"))
def test_scatter_add_rows_is_the_ascending_fp32_sum(c):
    M, L, st = _lib()
    inp = cb.inputs("scatter_add_rows", c)
    want = cb.impl("scatter_add_rows", c, inp, torch.float32)
    src, index = inp["src"].cuda(), inp["index"].cuda()
    dst = torch.zeros(int(inp["rows"]), c["C"], dtype=torch.float32, device="cuda")
    M.check(L.pp_scatter_add_rows(src.data_ptr(), index.data_ptr(), c["n"], c["C"], dst.data_ptr(), st), "pp_scatter_add_rows")
    assert torch.equal(dst.cpu(), want), cb.case_name("scatter_add_rows", c)
