"""The bounds of tests/corr_bounds.py discriminate (no GPU).  For every case of the sweep the independent fp32 CPU implementation (the
kernels' formula restated in torch float32, and in the emulated operand arithmetic of the f16x3 / f16 modes) stays inside the bound; its
worst |err| / model over the sweep is printed and is what the margins were set from (margin <= 4 x measured).  Every structurally wrong
variant, evaluated in float64 so that only the structural error remains, leaves the bound in at least one named case.  The exemption caps
hold for the float64 reference and the fp32 implementation alone, before any GPU is involved."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corr_bounds as cb  # noqa: E402

_CACHE = {}


def _model(op, c, mode="f32"):
    key = (cb.case_name(op, c), mode)
    if key not in _CACHE:
        inp = cb.inputs(op, c)
        _CACHE[key] = (inp, cb.model(op, c, inp, mode) if op == "corr" else cb.model(op, c, inp))
    return _CACHE[key]


def _margin_checks(key, worst, where):
    m = cb.MARGIN[key]
    print(f"[margin] {key}: fp32 CPU worst |err| / model = {worst:.3g} at {where}; margin {m:.3g} -> worst |err| / bound = {worst / m:.3g}")
    assert worst <= m, (key, worst, where)
    assert m <= 4.0 * worst, f"{key}: the margin {m} is more than 4 x the measured {worst:.3g}"


@pytest.mark.parametrize("mode", cb.MODES)
def test_forward_fp32_stays_inside(mode):
    worst, where = 0.0, None
    for c in cb.CASES["corr"]:
        inp, (ref, m) = _model("corr", c, mode)
        got = cb.impl("corr", c, inp, torch.float32, mode=mode)
        assert bool(torch.isfinite(got).all()), cb.case_name("corr", c)
        bad = cb._bad(inp["flow"])
        assert not bool(got[bad].any()) and not bool(ref[bad].any()) and not bool(m[bad].any())          # non-finite flow: exactly 0, never exempt
        assert not bool(got[(m == 0)].any()), cb.case_name("corr", c)                                   # four outside taps: exactly 0
        r = cb.worst_ratio(got, ref, m)
        if r > worst:
            worst, where = r, cb.case_name("corr", c)
    _margin_checks("corr:" + mode, worst, where)


def test_forward_wrong_variants_leave_the_bound():
    for w, rule in cb.WRONG["corr"].items():
        best, where = 0.0, None
        for c in cb.CASES["corr"]:
            if not rule(c):
                continue
            inp, (ref, m) = _model("corr", c)
            r = cb.worst_ratio(cb.impl("corr", c, inp, torch.float64, wrong=w), ref, m) / cb.MARGIN["corr:f32"]
            if r > best:
                best, where = r, cb.case_name("corr", c)
        print(f"[wrong]  corr / {w}: |err| / bound = {best:.3g} at {where}")
        assert best > 1.0, (w, best, where)


def test_pooled_axis_of_size_one_follows_the_reference():
    """On a pooled axis of size 1 every window offset samples coordinate 0: the float64 reference has equal samples along that axis and the
    restated formula agrees with it; the former formula (value only at offset 0) leaves the bound on every such case."""
    hit = 0
    for c in cb.CASES["corr"]:
        fx, fy = cb.flat_axes(c)
        if not (fx or fy) or c["kind"] in ("far", "nonfinite"):
            continue
        inp, (ref, m) = _model("corr", c)
        L, win = c["L"], 2 * c["r"] + 1
        last = ref[..., (L - 1) * win * win:].reshape(*ref.shape[:3], win, win)             # [a, b]
        same = last - (last[..., :1, :] if fx else last[..., :, :1])
        assert float(same.abs().max()) == 0.0 and float(last.abs().max()) > 0.0
        assert cb.worst_ratio(cb.impl("corr", c, inp, torch.float64), ref, m) <= cb.MARGIN["corr:f32"]
        assert cb.worst_ratio(cb.impl("corr", c, inp, torch.float64, wrong="flat_axis_as_today"), ref, m) > cb.MARGIN["corr:f32"]
        hit += 1
    assert hit >= 4


def test_adjoint_fp32_stays_inside_and_caps_hold():
    worst, where, worst_d, where_d = 0.0, None, 0.0, None
    for c in cb.CASES["corr_bwd"]:
        name = cb.case_name("corr_bwd", c)
        inp, (ref, m, md, near, jump) = _model("corr_bwd", c)
        got = cb.impl("corr_bwd", c, inp, torch.float32)
        assert not bool(jump[~near].any())
        # (the one-sided jump of a near-integer component is no rounding model and takes no margin: it is taken off the error first)
        e2 = ((got[2].double() - ref[2]).abs() - jump).clamp_min(0)
        got = (got[0], got[1], ref[2] + e2)
        bad = cb._bad(inp["flow"])
        for t in (got[0], got[2], ref[0], ref[2], m[0], m[2]):
            assert not bool(t[bad].any()), name                                                          # never exempt: exactly 0
        frac = float(near.double().mean())
        if c["kind"] not in cb.PLANTED:
            assert frac <= 0.01, f"{name}: {frac:.3%} of the dflow components fall under the near-integer rule"
        r = cb.worst_ratio(got, ref, m)
        if r > worst:
            worst, where = r, name
        # (the deterministic form differs in df2 alone; its fixed-point rounding is not restated: the same fp32 result against its model)
        rd = cb.worst_ratio(got, ref, md)
        if rd > worst_d:
            worst_d, where_d = rd, name
    _margin_checks("corr_bwd", worst, where)
    _margin_checks("corr_bwd_det", worst_d, where_d)


def test_adjoint_wrong_variants_leave_the_bound():
    for w, rule in cb.WRONG["corr_bwd"].items():
        best, where = 0.0, None
        for c in cb.CASES["corr_bwd"]:
            if not rule(c) or c["H"] * c["W"] > 512:
                continue
            inp, (ref, m, _, _, _) = _model("corr_bwd", c)
            r = cb.worst_ratio(cb.impl("corr_bwd", c, inp, torch.float64, wrong=w), ref, m) / cb.MARGIN["corr_bwd"]
            if r > best:
                best, where = r, cb.case_name("corr_bwd", c)
        print(f"[wrong]  corr_bwd / {w}: |err| / bound = {best:.3g} at {where}")
        assert best > 1.0, (w, best, where)


def test_adjoint_on_a_pooled_axis_of_size_one_is_exactly_zero_in_the_reference():
    hit = 0
    for c in cb.CASES["corr_bwd"]:
        fx, fy = cb.flat_axes(c)
        if not (fx or fy):
            continue
        inp, (ref, _, _, _, _) = _model("corr_bwd", c)
        # the last level contributes nothing along the flat axis: the reference gradient equals that of the lookup without the level
        c2 = dict(c, L=c["L"] - 1)
        win2 = (c["L"] - 1) * (2 * c["r"] + 1) ** 2
        ref2, _, _, _, _ = cb.model("corr_bwd", c2, dict(inp, dout=inp["dout"][..., :win2].contiguous()))
        axis = 0 if fx else 1
        assert torch.equal(ref[2][..., axis], ref2[2][..., axis]), cb.case_name("corr_bwd", c)
        hit += 1
    assert hit >= 2


# ------------------------------------------------------------------------------------------------------------------ the loss kernels
def _strip(op, got, out):
    """take the exemptions' allowance (no rounding model: it takes no margin) off the error before it is measured against the model"""
    ref, extra = out[0], out[2]
    if op == "flow_loss":
        return ref + ((got.double() - ref).abs() - extra).clamp_min(0)
    return tuple(r + ((g.double() - r).abs() - x).clamp_min(0) for g, r, x in zip(got, ref, extra))


@pytest.mark.parametrize("op", cb.LOSS_OPS)
def test_loss_kernels_fp32_stays_inside_and_wrong_variants_leave(op):
    worst, where = 0.0, None
    wrong = cb.WRONG.get(op, {})
    best = {w: (0.0, None) for w in wrong}
    for c in cb.CASES[op]:
        name = cb.case_name(op, c)
        inp = cb.inputs(op, c)
        out = cb.model(op, c, inp)
        ref, m = out[0], out[1]
        got = cb.impl(op, c, inp, torch.float32)
        if op.startswith("flow_loss"):
            got = _strip(op, got, out)
        r = cb.worst_ratio(got, ref, m)
        if r > worst:
            worst, where = r, name
        _, bound = cb.reference(op, c, inp)
        for w, rule in wrong.items():
            if not rule(c):
                continue
            dt = torch.float32 if (op, w) in cb.WRONG_IN_FP32 else torch.float64
            gw = cb.impl(op, c, inp, dt, wrong=w)
            rw = cb.worst_ratio(gw, ref, bound)
            if rw > best[w][0]:
                best[w] = (rw, name)
    for w in wrong:
        print(f"[wrong]  {op} / {w}: |err| / bound = {best[w][0]:.3g} at {best[w][1]}")
        assert best[w][0] > 1.0, (op, w, best[w])
    if cb.MARGIN[op] > 0:
        _margin_checks(op, worst, where)
    else:
        print(f"[margin] {op}: exact")
        assert worst == 0.0, (op, worst, where)


def test_loss_kernel_edges_and_exemption_caps():
    """The planted rows and pixels are decided exactly in the float64 reference and in the fp32 restatement, and no case exempts more than
    0.1 % of its positions from a threshold or a sign decision."""
    for c in cb.CASES["gather_normalize"]:
        inp = cb.inputs("gather_normalize", c)
        ref, m = cb.model("gather_normalize", c, inp)
        got = cb.impl("gather_normalize", c, inp, torch.float32)
        assert not bool(ref[0].any()) and not bool(got[0].any()) and not bool(m[0].any())                  # the zero row
        if c["n"] >= 3:
            assert abs(float(ref[1].norm()) - 1e-8) < 1e-12 and abs(float(ref[2].norm()) - 1.0) < 1e-9       # |x| = 1e-20 / eps, |x| = 1e-10
    for c in cb.CASES["xent_diag"]:
        inp = cb.inputs("xent_diag", c)
        ref, m = cb.model("xent_diag", c, inp)
        got = cb.impl("xent_diag", c, inp, torch.float32)
        if c["n"] == 1:
            assert float(got[0]) == 0.0 and float(ref[0]) == 0.0
        if c["n"] > 8:     # the dominated rows: losses of ~7e-3 n, ~2e-9 n and < 1e-33, where only the absolute model decides
            assert 1e-4 < float(ref[0]) < 10 and float(ref[1]) < 1e-5 and float(ref[2]) < 1e-30
            assert float(got[2]) == 0.0
            assert float(m[1]) > 100 * float(ref[1])
    for op in ("flow_loss", "flow_loss_bwd"):
        for c in cb.CASES[op]:
            name = cb.case_name(op, c)
            inp = cb.inputs(op, c)
            out = cb.model(op, c, inp)
            B, H, W = c["B"], c["H"], c["W"]
            planted = c["fill"] != "none" and H >= 16
            if op == "flow_loss":
                ref, edge = out[0], out[3]
                assert float(edge.double().mean()) <= 1e-3, name
                got = cb.impl(op, c, inp, torch.float32)
                assert float(got[2]) == float(ref[2]) or bool(edge.any()), name                                # the count is exact
                if c["fill"] == "none":
                    assert float(ref[1]) == 0.0 and float(ref[2]) == 0.0 and float(got[1]) == 0.0
                if planted:
                    assert not bool(edge[B - 1, 0, 0]), name                                                   # the exact tie is not exempt
            else:
                (dfl, _), (edge, sign_free) = out[0], out[3]
                assert float(edge.double().mean()) <= 1e-3 and float(sign_free.double().mean()) <= 1e-3, name
                got = cb.impl(op, c, inp, torch.float32)[0]
                assert set(torch.unique(dfl / float(inp["gf"][0])).round().tolist()) <= {-1.0, 0.0, 1.0}
                if planted:
                    assert not bool(sign_free[B - 1, 0, W - 1].any()) and not bool(edge[B - 1, 0, 0])
                    assert not bool(dfl[B - 1, 0, W - 1].any()) and not bool(got[B - 1, 0, W - 1].any())       # flow == fl32(g): exactly 0
                    assert not bool(dfl[B - 1, 0, 0].any()) and not bool(got[B - 1, 0, 0].any())               # |g| == max_flow: not < max_flow
