"""The float64 bound of tests/engine_bounds.py discriminates (no GPU): a numpy emulation of the engine's operand formats —
activation hi / lo = f16(4 x), f16(4 x - hi) saturated at +-65504 with fp16 subnormals; weights scaled by 2^e, e clamped to
+-30; the product hi.hi + hi.lo + lo.hi evaluated in float64 — stays inside the f16x3 bound, while the 2-term products (the
activation's or the weight's lo term dropped: what -DPP_STUDY_ACT_LO_ZERO / -DPP_STUDY_W_LO_ZERO build) and the plain-fp16
1-term product violate it on every shape of the GPU sweep with at least 64 outputs.  The 1-term product stays inside the f16
bound."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_bounds as eb  # noqa: E402

DENSE = eb.DENSE


def split_act(x):
    """f16x3 activation operand (csrc/pp_common.h pp_split_f16): (hi, lo) as float64 arrays of the fp16 values, scale 4."""
    a = (x.astype(np.float32) * np.float32(4.0)).astype(np.float32)
    hi = np.clip(a, -65504, 65504).astype(np.float16)
    lo = np.clip(a - hi.astype(np.float32), -65504, 65504).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def split_weight(w):
    """f16x3 weight operand (pp_split_weights_t): (hi, lo, s) of s w, s = 2^e."""
    s = np.float32(2.0 ** eb.weight_exponent(torch.from_numpy(w)))
    a = (w.astype(np.float32) * s).astype(np.float32)
    hi = np.clip(a, -65504, 65504).astype(np.float16)
    lo = (a - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64), float(s)


def emulate(x, w):
    """{name: x @ w.T in float64 from the operand terms}: "3" (hi.hi + hi.lo + lo.hi), "2a" (activation lo dropped), "2w"
    (weight lo dropped), "1" (hi.hi: the plain-fp16 "h" operands of the f16 mode)."""
    ah, al = split_act(x)
    wh, wl, s = split_weight(w)
    d = 4.0 * s
    hh, hl, lh = ah @ wh.T, ah @ wl.T, al @ wh.T
    return {"3": (hh + hl + lh) / d, "2a": (hh + hl) / d, "2w": (hh + lh) / d, "1": hh / d}


def _data(M, K, N):
    g = torch.Generator().manual_seed(M * 7 + K * 3 + N)
    return torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5


@pytest.mark.parametrize("M,K,N", DENSE)
def test_emulated_operand_formats_against_the_bound(M, K, N):
    x, w = _data(M, K, N)
    em = emulate(x.numpy(), w.numpy())
    ref3, bound3 = eb.reference("linear", x, w, "f16x3")
    ref1, bound1 = eb.reference("linear", x, w, "f16")
    ratio = {k: float(((torch.from_numpy(v) - ref3).abs() / bound3).max()) for k, v in em.items()}
    r1_f16 = float(((torch.from_numpy(em["1"]) - ref1).abs() / bound1).max())
    print(f"[emulation] M={M} K={K} N={N}: |err|/bound(f16x3) 3-term {ratio['3']:.3g}, 2-term act-lo {ratio['2a']:.3g}, "
          f"2-term w-lo {ratio['2w']:.3g}, 1-term {ratio['1']:.3g}; 1-term / bound(f16) {r1_f16:.3g}")
    assert ratio["3"] <= 1.0, ratio
    assert r1_f16 <= 1.0, r1_f16
    if M * N >= 64:
        for k in ("2a", "2w", "1"):
            assert ratio[k] > 1.0, (k, ratio)


def test_weight_exponent_rule():
    """The weight-scale rule of pp_split_weights_ws: s max|w| in [512, 1024), clamp +-30, 0 for an all-zero weight."""
    for m in (1.0, 0.75, 2.0 ** -20, 2.0 ** 20, 1000.0, 3e-3):
        e = eb.weight_exponent(torch.tensor([m, -m / 3]))
        assert 512 <= m * 2.0 ** e < 1024, (m, e)
    assert eb.weight_exponent(torch.tensor([2.0 ** -40])) == 30
    assert eb.weight_exponent(torch.tensor([2.0 ** 40])) == -30
    assert eb.weight_exponent(torch.zeros(8)) == 0
    one_below = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    assert eb.weight_exponent(torch.tensor([1.0])) == 9 and eb.weight_exponent(torch.tensor([one_below])) == 10


def test_activation_floor_below_two_to_the_minus_five():
    """f16x3 keeps 22 bits for |x| >= 2^-5 and an absolute floor of 2^-27 per element below (the contract DESIGN.md states)."""
    rng = np.random.default_rng(0)
    for lo_exp, hi_exp in ((-5, 13), (-40, -5)):
        x = (rng.uniform(1, 2, 200000) * 2.0 ** rng.integers(lo_exp, hi_exp, 200000) * rng.choice([-1, 1], 200000)).astype(np.float32)
        h, l = split_act(x)
        err = np.abs((h + l) / 4 - x.astype(np.float64))
        assert (err <= 2.0 ** -22 * np.abs(x) + 2.0 ** -27).all()
        if lo_exp == -5:
            assert (err <= 2.0 ** -22 * np.abs(x)).all()
        else:
            assert err.max() > 2.0 ** -22 * np.abs(x[err.argmax()])      # the floor binds down there
    h, _ = split_act(np.array([16370.0, 16400.0], np.float32))
    assert abs(h[0]) < 65504 and h[1] == 65504                              # the saturation limit |x| < 16376
