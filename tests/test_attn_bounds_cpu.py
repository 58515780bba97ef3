"""The bounds of tests/attn_bounds.py discriminate (no GPU).  For every case of the sweep the kernels' formula restated in torch float32 (the
chunked online soft-max of the f32 kernel, and the emulated operand splits of the f16x3 / f16 modes and of the adjoint) stays inside the bound;
its worst |err| / model over the sweep is printed and is what the margins were set from (margin <= 4 x measured, held to [margin / 4, margin]
on whichever host this runs).  Every structurally wrong variant, evaluated in float64 with the quantisers kept so that only the structural
error remains, leaves the bound at its named case and stays inside wherever its rule says it cannot show.  The float64 reference's own
identities hold before any GPU is involved."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_bounds as ab  # noqa: E402

_CACHE = {}


def _model(op, c, mode="f32"):
    key = (ab.case_name(op, c), mode)
    if key not in _CACHE:
        inp = ab.inputs(op, c)
        _CACHE[key] = (inp, ab.model(op, c, inp, mode))
    return _CACHE[key]


def _margin_checks(key, worst, where):
    m = ab.MARGIN[key]
    print(f"[margin] {key}: fp32 CPU worst |err| / model = {worst:.3g} at {where}; margin {m:.3g} -> worst |err| / bound = {worst / m:.3g}")
    assert worst <= m, (key, worst, where)
    assert m <= 4.0 * worst, f"{key}: the margin {m} is more than 4 x the measured {worst:.3g}"


@pytest.mark.parametrize("mode", ab.MODES)
def test_forward_stays_inside(mode):
    worst, where = 0.0, None
    for c in ab.CASES["attn"]:
        inp, (ref, m) = _model("attn", c, mode)
        got = ab.impl("attn", c, inp, torch.float32, mode)
        assert bool(torch.isfinite(got).all()), ab.case_name("attn", c)
        r = ab.worst_ratio(got, ref, m)
        if r > worst:
            worst, where = r, ab.case_name("attn", c)
    _margin_checks("attn:" + mode, worst, where)


def test_log_sum_exp_stays_inside():
    worst, where = 0.0, None
    for c in ab.CASES["attn_lse"]:
        inp, (ref, m) = _model("attn_lse", c)
        got = ab.impl("attn_lse", c, inp, torch.float32)
        assert bool(torch.isfinite(got).all()), ab.case_name("attn_lse", c)
        r = ab.worst_ratio(got, ref, m)
        if r > worst:
            worst, where = r, ab.case_name("attn_lse", c)
    _margin_checks("attn_lse", worst, where)


def test_adjoint_stays_inside():
    worst = {k: (0.0, None) for k in ab.BWD_KEYS}
    for c in ab.CASES["attn_bwd"]:
        inp, (ref, m) = _model("attn_bwd", c)
        got = ab.impl("attn_bwd", c, inp, torch.float32)
        for key, g, r_, m_ in zip(ab.BWD_KEYS, got, ref, m):
            assert bool(torch.isfinite(g).all()), (key, ab.case_name("attn_bwd", c))
            r = ab.worst_ratio(g, r_, m_)
            if r > worst[key][0]:
                worst[key] = (r, ab.case_name("attn_bwd", c))
    for key in ab.BWD_KEYS:
        _margin_checks(key, *worst[key])


def _bound_ratio(op, c, got, mode):
    """worst |got - ref| / bound of a float64 variant (the adjoint: over dq, dk, dv with their own margins)"""
    _, (ref, m) = _model(op, c, mode)
    if op == "attn_bwd":
        return max(ab.worst_ratio(g, r_, m_) / ab.MARGIN[key] for key, g, r_, m_ in zip(ab.BWD_KEYS, got, ref, m))
    return ab.worst_ratio(got, ref, m) / ab.MARGIN["attn:" + mode if op == "attn" else op]


@pytest.mark.parametrize("op", ab.OPS)
def test_wrong_variants_leave_the_bound_where_their_rule_says(op):
    for w, (broken, rule, _) in ab.WRONG[op].items():
        modes = ("f16x3",) if (op != "attn" or w in ("p_lo_dropped", "lohi_dropped")) else ("f32", "f16x3")
        named = ab.named(op, w)
        assert named, (op, w)
        for mode in modes:
            best, where, quiet = 0.0, None, 0.0
            for c in ab.CASES[op]:
                inp, _ = _model(op, c, mode)
                r = _bound_ratio(op, c, ab.impl(op, c, inp, torch.float64, mode, wrong=w), mode)
                if not rule(c):
                    quiet = max(quiet, r)
                    assert r <= 1.0, f"{op} / {w} ({mode}) leaves the bound at {ab.case_name(op, c)}, where its rule says it cannot show: {r:.3g}"
                elif c in named:
                    print(f"[wrong]  {op} / {w} ({mode}; {broken}): |err| / bound = {r:.3g} at {ab.case_name(op, c)}")
                    assert r > 1.0, (op, w, mode, r, ab.case_name(op, c))
                if rule(c) and r > best:
                    best, where = r, ab.case_name(op, c)
            print(f"[wrong]  {op} / {w} ({mode}): largest |err| / bound = {best:.3g} at {where}; where the rule excludes it: {quiet:.3g}")


def test_dropped_lo_term_of_p_stays_inside_the_f16_bound():
    """P with one fp16 term is what the f16 mode computes: outside the f16x3 bound (above), inside the f16 bound at every case"""
    worst = 0.0
    for c in ab.CASES["attn"]:
        inp, (ref, m) = _model("attn", c, "f16")
        got = ab.impl("attn", c, inp, torch.float64, "f16x3", wrong="p_lo_dropped")
        worst = max(worst, ab.worst_ratio(got, ref, m) / ab.MARGIN["attn:f16"])
    print(f"[wrong]  attn / p_lo_dropped against the f16 bound: |err| / bound = {worst:.3g}")
    assert worst <= 1.0


def test_correct_formula_in_float64_with_the_quantisers_is_inside():
    """the structural errors above are measured against this: the same restatement without an error stays well inside"""
    for op in ab.OPS:
        for c in ab.CASES[op]:
            inp, _ = _model(op, c, "f16x3")
            r = _bound_ratio(op, c, ab.impl(op, c, inp, torch.float64, "f16x3"), "f16x3")
            assert r <= 1.0, (op, ab.case_name(op, c), r)


def test_unfused_chain_restated_in_fp32_fits_the_fused_bounds():
    """S = q k^T / 8, the row soft-max, P v and the adjoint from the kept P, in torch float32: inside the f32 forward bound and the adjoint's
    bounds, so the GPU test holds the unfused chain to the same references and bounds as the fused kernels"""
    worst = {}
    for c in ab.UNFUSED:
        inp, (ref, m) = _model("attn_bwd", c)
        got = ab.impl("attn_bwd", c, inp, torch.float32, "unfused")
        for key, g, r_, m_ in zip(ab.BWD_KEYS, got, ref, m):
            worst[key] = max(worst.get(key, 0.0), ab.worst_ratio(g, r_, m_) / ab.MARGIN[key])
        ref, m = ab.model("attn", c, inp, "f32")
        worst["attn:f32"] = max(worst.get("attn:f32", 0.0), ab.worst_ratio(ab.impl("attn", c, inp, torch.float32, "unfused"), ref, m) / ab.MARGIN["attn:f32"])
    for key, r in worst.items():
        print(f"[unfused] {key}: fp32 restatement of the unfused chain, worst |err| / bound = {r:.3g}")
        assert r <= 1.0, (key, r)


def test_unfused_f16x3_adjoint_has_margins_of_its_own():
    """FUSED_ATTENTION off in f16x3: dS is split with one power of two for the whole tensor, the kept P at scale 4.  The chain's restatement with
    the emulated splits leaves the FUSED dk bound at the peaked case (a key that receives little attention) and sets the margins of the chain's
    own model"""
    worst = {k: (0.0, None) for k in ab.UNFUSED_KEYS}
    fused_dk = 0.0
    for c in ab.UNFUSED:
        inp, (ref, mf) = _model("attn_bwd", c)
        _, m = ab.model("attn_bwd", c, inp, unfused=True)
        got = ab.impl("attn_bwd", c, inp, torch.float32, "unfused_f16x3")
        for i, key in enumerate(ab.UNFUSED_KEYS):
            r = ab.worst_ratio(got[i], ref[i], m[i])
            if r > worst[key][0]:
                worst[key] = (r, ab.case_name("attn_bwd", c))
        fused_dk = max(fused_dk, ab.worst_ratio(got[1], ref[1], mf[1]) / ab.MARGIN["attn_bwd:dk"])
    print(f"[unfused] the f16x3 chain's dk against the fused bound: |err| / bound = {fused_dk:.3g}")
    assert fused_dk > 1.0
    for key in ab.UNFUSED_KEYS:
        _margin_checks(key, *worst[key])


def test_reference_identities():
    """rows of p sum to 1; T = 1: out = v, dq = dk = 0, dv = dout; the case list covers what the issue asks of it"""
    for c in ab.CASES["attn"]:
        inp = ab.inputs("attn", c)
        out, lse, p = ab.ref_forward(inp["qkv"].double(), c)
        assert float((p.sum(-1) - 1).abs().max()) <= 1e-14, ab.case_name("attn", c)
        if c["T"] == 1:
            C = c["heads"] * ab.HD
            assert torch.equal(out, inp["qkv"][:, 2 * C:].double())
            assert torch.equal(ab.impl("attn", c, inp, torch.float32, "f32"), inp["qkv"][:, 2 * C:])
    seen = 0
    for c in ab.CASES["attn_bwd"]:
        if c["T"] != 1:
            continue
        inp, ((dq, dk, dv), m) = _model("attn_bwd", c)
        assert not bool(dq.any()) and not bool(dk.any()) and torch.equal(dv, inp["dout"].double())
        seen += 1
    assert seen >= 1
    fwd = ab.CASES["attn"]
    assert {c["T"] for c in fwd if c["kind"] == "normal"} == set(ab.TS)
    for kind in ab.KINDS:
        ts = {c["T"] for c in fwd if c["kind"] == kind}
        assert 37 in ts and 257 in ts and any(t <= 4 for t in ts), kind
    assert {c["B"] * c["heads"] for c in fwd} >= {1, 3, 8, 9}
    assert all(c["heads"] <= 3 for c in fwd if c["T"] >= 257) and all(c["T"] <= 129 for c in fwd if c["B"] * c["heads"] == 9)
    assert {c["dout"] for c in ab.CASES["attn_bwd"]} == set(ab.DOUTS)
