"""The bounds of tests/kernel_bounds.py discriminate (no GPU).  For every operation and every case of the sweep the independent
fp32 CPU implementation (the kernel's formula restated in torch float32) stays inside the bound — its worst |err| / model over the
sweep is what the margins were set from, and is printed — and every structurally wrong implementation, evaluated in float64 so
that only the structural error remains, leaves it on every case whose size rule says the case contains the error.  No (operation,
wrong implementation) pair may be exempt on more than a quarter of the operation's cases."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_bounds as kb  # noqa: E402


@pytest.mark.parametrize("op", kb.OPS)
def test_fp32_stays_inside_and_wrong_arithmetic_leaves(op):
    worst32, worst_case = 0.0, None
    wrong = kb.WRONG.get(op, {})
    asserted = {w: 0 for w in wrong}
    least = {w: float("inf") for w in wrong}
    cases = kb.CASES[op]
    for c in cases:
        inp = kb.inputs(op, c)
        ref, m = kb.model(op, c, inp)
        r = kb.worst_ratio(kb.impl(op, c, inp, torch.float32), ref, m)
        if r > worst32:
            worst32, worst_case = r, kb.case_name(op, c)
        r64 = kb.worst_ratio(kb.impl(op, c, inp, torch.float64), ref, m)      # the restated formula itself agrees with torch's op
        assert r64 <= kb.MARGIN[op] / 2, (kb.case_name(op, c), r64)   # (softmax adjoint: its fp32 probabilities are an input)
        for w, rule in wrong.items():
            if not rule(c):
                continue
            rw = kb.worst_ratio(kb.impl(op, c, inp, torch.float64, wrong=w), ref, m) / kb.MARGIN[op] if kb.MARGIN[op] > 0 else float("inf")
            asserted[w] += 1
            least[w] = min(least[w], rw)
            assert rw > 1.0, f"{kb.case_name(op, c)}: wrong implementation {w!r} stays inside the bound (|err| / bound = {rw:.3g})"
    print(f"[margin] {op}: fp32 CPU worst |err| / model = {worst32:.3g} at {worst_case}; margin {kb.MARGIN[op]:.3g} "
          f"-> worst |err| / bound = {worst32 / kb.MARGIN[op] if kb.MARGIN[op] else 0:.3g}")
    for w in wrong:
        print(f"[wrong]  {op} / {w}: asserted on {asserted[w]} of {len(cases)} cases, least |err| / bound = {least[w]:.3g}")
        assert len(cases) - asserted[w] <= len(cases) // 4, (op, w, asserted[w], len(cases))
    if kb.MARGIN[op] > 0:
        assert worst32 <= kb.MARGIN[op], (op, worst32, worst_case)
        assert worst32 >= kb.MARGIN[op] / 4, f"{op}: the margin {kb.MARGIN[op]} is more than 4 x the measured {worst32:.3g}"
    else:
        assert worst32 == 0.0, (op, worst32, worst_case)       # an exact operation: bit-equal


def test_warp_adjoint_bound_rejects_a_gradient_along_an_axis_of_size_one():
    """pp_warp_backward_nhwc once handed dflow on along an axis of size 1, where the coordinate round trip multiplies by size - 1 = 0 and
    the gradient is exactly 0.  That formula leaves the bound on both degenerate cases of the sweep (outside WRONG: only those two
    cases of the operation can contain the error, so the one-quarter cap on exemptions does not fit it)."""
    hit = 0
    for c in kb.CASES["warp_bwd"]:
        if c["H"] > 1 and c["W"] > 1:
            continue
        inp = kb.inputs("warp_bwd", c)
        ref, bound = kb.reference("warp_bwd", c, inp)
        axis = 1 if c["H"] == 1 else 0
        assert float(ref[1][..., axis].abs().max()) == 0.0 and float(bound[1][..., axis].max()) == 0.0
        assert kb.worst_ratio(kb.impl("warp_bwd", c, inp, torch.float32), ref, bound) <= 1.0
        r = kb.worst_ratio(kb.impl("warp_bwd", c, inp, torch.float64, wrong="degenerate_axis_gradient"), ref, bound)
        print(f"[wrong]  {kb.case_name('warp_bwd', c)} / degenerate_axis_gradient: |err| / bound = {r:.3g}")
        assert r > 1.0
        hit += 1
    assert hit >= 2


def test_sweep_data_reaches_the_edges():
    """The warp flows put every one of the 9 border situations (inside, 4 edges, 4 corners; plus fully outside) at >= 1 % each."""
    for c in kb.CASES["warp"]:
        if c["kind"] != "border" or c["H"] * c["W"] * c["B"] < 1500:
            continue
        fl = kb.inputs("warp", c)["flow"].double()
        iy, ix = kb._warp_coords(c, fl, torch.float64)
        H, W = c["H"], c["W"]
        sx = torch.where(ix < 0, 0, torch.where(ix > W - 1, 2, 1))
        sy = torch.where(iy < 0, 0, torch.where(iy > H - 1, 2, 1))
        outside = (ix <= -1) | (ix >= W) | (iy <= -1) | (iy >= H)
        assert float(outside.double().mean()) >= 0.01
        for a in range(3):
            for b in range(3):
                if H == 1 and a != 1:
                    continue
                frac = float(((sx == b) & (sy == a) & ~outside).double().mean())
                assert frac >= 0.01, (kb.case_name("warp", c), a, b, frac)
