"""The bounds of tests/wino_bounds.py discriminate (no GPU).  For every case of the sweep the kernels' expression order restated in torch
float32 (for F(4x4) with the emulated operand arithmetic) stays inside the bound, element by element with no share of elements left out;
its worst |err| / model over the sweep is printed and is what the margins were set from (margin <= 4 x measured).  Every structurally wrong
variant, evaluated in float64 so that only the structural error remains, leaves the bound in at least one named case; the variants that
confuse H and W do so on non-square maps only.  The exactness conditions hold for the float64 reference and the fp32 restatement."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wino_bounds as wb  # noqa: E402

_CACHE = {}


def _model(op, c):
    key = wb.case_name(op, c)
    if key not in _CACHE:
        inp = wb.inputs(op, c)
        _CACHE[key] = (inp, wb.model(op, c, inp))
    return _CACHE[key]


@pytest.mark.parametrize("op", [op for op in wb.CASES])
def test_fp32_restatement_stays_inside(op):
    worst, where = 0.0, None
    for c in wb.CASES[op]:
        inp, (ref, m, fixed) = _model(op, c)
        got = wb.impl(op, c, inp, torch.float32)
        for g_ in (got if isinstance(got, tuple) else (got,)):
            assert bool(torch.isfinite(g_).all()), wb.case_name(op, c)
        r = wb.excess_ratio(got, ref, m, fixed)
        if r > worst:
            worst, where = r, wb.case_name(op, c)
    mg = wb.MARGIN[wb.MARGIN_OF.get(op, op)]
    if op in wb.MARGIN_OF:      # composed from the stages' margins: inside, with no margin of its own to set
        print(f"[margin] {op}: fp32 CPU worst |err| / model = {worst:.3g} at {where}; margin of {wb.MARGIN_OF[op]} {mg:.3g} -> worst |err| / bound = {worst / mg:.3g}")
        assert worst <= mg, (op, worst, where)
        return
    print(f"[margin] {op}: fp32 CPU worst |err| / model = {worst:.3g} at {where}; margin {mg:.3g} -> worst |err| / bound = {worst / mg:.3g}")
    assert worst <= mg, (op, worst, where)
    assert mg <= 4.0 * worst, f"{op}: the margin {mg} is more than 4 x the measured {worst:.3g}"


def test_wrong_variants_leave_the_bound():
    for op, variants in wb.WRONG.items():
        for w, rule in variants.items():
            best, where = 0.0, None
            for c in wb.CASES[op]:
                square = c["H"] == c["W"]
                if not rule(c) and not (w in wb.ONLY_NONSQUARE and square):
                    continue
                inp, (ref, m, fixed) = _model(op, c)
                r = wb.excess_ratio(wb.impl(op, c, inp, torch.float64, wrong=w), ref, m, fixed) / wb.MARGIN[wb.MARGIN_OF.get(op, op)]
                if w in wb.ONLY_NONSQUARE and square:
                    assert r <= 1.0, f"{op} / {w} shows on the square case {wb.case_name(op, c)}: {r:.3g}"
                    continue
                if r > best:
                    best, where = r, wb.case_name(op, c)
            shown = f"{best:.3g}" if best < 1e100 else "inf (an element whose bound is 0)"
            print(f"[wrong]  {op} / {w}: |err| / bound = {shown} at {where}")
            assert best > 1.0, (op, w, best, where)


def test_float64_restatement_is_inside_a_thousandth_of_every_bound():
    """the restated formula is the reference's function: in float64 only 1e-16-level rounding (and, for F(4x4), the operand split) remains"""
    for op in ("in2", "wt2", "wt4", "out2", "conv_w2", "chain2"):
        for c in wb.CASES[op]:
            inp, (ref, m, fixed) = _model(op, c)
            r = wb.excess_ratio(wb.impl(op, c, inp, torch.float64), ref, m, fixed)
            assert r <= 1e-3, (wb.case_name(op, c), r)


def test_exactness_conditions():
    hit = {"zero_tile": 0, "dead": 0, "impulse": 0}
    for op in ("in2", "in4"):
        for c in wb.CASES[op]:
            inp, (ref, m, _) = _model(op, c)
            got = wb.impl(op, c, inp, torch.float32)
            zero = m == 0
            assert not bool(ref[zero].any()) and not bool(got[zero].any()), wb.case_name(op, c)          # a zero window: exactly 0
            if c["kind"] == "sparse":
                hit["zero_tile"] += int(zero.all(0).all(-1).any())
            if c["kind"] == "dead":
                assert bool(zero.all()), wb.case_name(op, c)
                hit["dead"] += 1
    for c in wb.CASES["conv_w2"]:
        inp, (ref, m, _) = _model("conv_w2", c)
        if c["kind"] == "dead":
            # nothing passes the input ReLU: act(bias) + residuals, exactly (the fp32 sums of the epilogue in its order)
            want = wb._act(inp["bias"] if "bias" in inp else torch.zeros(c["Cout"]), c["act"]).expand(c["B"], c["H"], c["W"], -1)
            for k in ("r1", "r2"):
                if k in inp:
                    want = want + inp[k]
            assert torch.equal(wb.impl("conv_w2", c, inp, torch.float32), want), wb.case_name("conv_w2", c)
            hit["dead"] += 1
    for op in ("conv_w2", "conv_w4"):
        for c in wb.CASES[op]:
            if c["kind"] != "impulse" or c["relu_in"] or c.get("hl") or c.get("also"):
                continue
            # a one-hot tap: the float64 pre-activation is the input shifted by (+1, -1), channel co % Cin
            inp = dict(wb.inputs(op, c))
            for k in ("bias", "r1", "r2"):
                inp.pop(k, None)
            cc = dict(c, act=None, nres=0, bias=False)
            ref = wb.model(op, cc, inp)[0]
            x = inp["x"].double()
            want = torch.zeros_like(ref)
            want[:, 1:, :-1, :] = x[:, :-1, 1:, torch.arange(c["Cout"]) % c["Cin"]]
            assert torch.equal(ref, want), wb.case_name(op, c)
            got = wb.impl(op, cc, inp, torch.float64)
            assert float((got - want).abs().max()) <= (1e-12 if op == "conv_w2" else 2.0 ** -20 * float(want.abs().max())), wb.case_name(op, c)
            hit["impulse"] += 1
    assert all(v >= 2 for v in hit.values()), hit
