"""The bounds of tests/geom_bounds.py discriminate (no GPU).  For every operation and every case of the sweep the independent fp32
CPU implementation (the kernel's formula restated in torch float32) stays inside the bound — its worst |err| / model over the sweep
is what the margins were set from, and is printed — and every structurally wrong implementation leaves it on every case whose rule
says the case contains the error (in float64, so that only the structural error remains; the bit-equal operations in float32, where
"inside" means equal).  No (operation, wrong implementation) pair may be exempt on more than a quarter of the operation's cases,
except the two stage-3 variants that only a non-square map, resp. only the planted c = 0 against thr = 0.5 can show."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geom_bounds as gb  # noqa: E402

NARROW = {("stage3", "bounds_swapped"): 3, ("stage3", "ge"): 3, ("gather", "base_dropped"): 4}   # least number of cases that must show it


@pytest.mark.parametrize("op", gb.OPS)
def test_fp32_stays_inside_and_wrong_arithmetic_leaves(op):
    worst32, worst_case = 0.0, None
    wrong = gb.WRONG[op]
    asserted = {w: 0 for w in wrong}
    least = {w: float("inf") for w in wrong}
    cases = gb.CASES[op]
    exact = op in gb.EXACT
    for c in cases:
        inp = gb.inputs(op, c)
        ref, m = gb.model(op, inp)
        r = gb.ratio(op, gb.impl(op, inp, torch.float32), ref, m)
        if r > worst32:
            worst32, worst_case = r, gb.case_name(op, c)
        if not exact:            # the restated formula itself agrees with torch's float64 ops
            r64 = gb.ratio(op, gb.impl(op, inp, torch.float64), ref, m)
            assert r64 <= gb.MARGIN[op] / 2, (gb.case_name(op, c), r64)
        for w, rule in wrong.items():
            if not rule(c):
                continue
            rw = gb.ratio(op, gb.impl(op, inp, torch.float32 if exact else torch.float64, wrong=w), ref, m)
            rw = rw / gb.MARGIN[op] if not exact else rw
            asserted[w] += 1
            least[w] = min(least[w], rw)
            assert rw > 1.0, f"{gb.case_name(op, c)}: wrong implementation {w!r} stays inside the bound (|err| / bound = {rw:.3g})"
    print(f"[margin] {op}: fp32 CPU worst |err| / model = {worst32:.3g} at {worst_case}; margin {gb.MARGIN[op]:.3g} "
          f"-> worst |err| / bound = {worst32 / gb.MARGIN[op] if gb.MARGIN[op] else 0:.3g}")
    for w in wrong:
        print(f"[wrong]  {op} / {w}: asserted on {asserted[w]} of {len(cases)} cases, least |err| / bound = {least[w]:.3g}")
        if (op, w) in NARROW:
            assert asserted[w] >= NARROW[(op, w)], (op, w, asserted[w])
        else:
            assert len(cases) - asserted[w] <= len(cases) // 4, (op, w, asserted[w], len(cases))
    if not exact:
        assert worst32 <= gb.MARGIN[op], (op, worst32, worst_case)
        assert worst32 >= gb.MARGIN[op] / 4, f"{op}: the margin {gb.MARGIN[op]} is more than 4 x the measured {worst32:.3g}"
        assert abs(worst32 - gb.MEASURED[op]) <= 0.02 * gb.MEASURED[op] + 1e-3, (op, worst32, gb.MEASURED[op])
    else:
        assert gb.MARGIN[op] == 0.0 and worst32 == 0.0, (op, worst32, worst_case)       # an exact operation: bit-equal


def test_stage3_exempt_share_is_under_its_cap_and_no_planted_position_is_exempt():
    """The band |sigmoid64(c) - thr| <= 8 u exempts at most 0.1 % of a case's positions and none of the planted ones; the fp32
    restatement decides every other position like float64 (asserted above); the plants are where they are meant to be."""
    planted_cases = 0
    for c in gb.CASES["stage3"]:
        inp = gb.inputs("stage3", c)
        (tar, src), b = gb.model("stage3", inp)
        share = float(b["exempt"].double().mean())
        print(f"[exempt] {gb.case_name('stage3', c)}: {int(b['exempt'].sum())} of {b['exempt'].numel()} positions ({share:.2e}); "
              f"kept {float((tar[..., 0] >= 0).double().mean()):.2f}")
        assert share <= gb.EXEMPT_CAP, (gb.case_name("stage3", c), share)
        for (bi, h, w) in inp["planted"]:
            assert not bool(b["exempt_bhw"][bi, h, w]), (gb.case_name("stage3", c), h, w)
        if not inp["planted"]:
            assert c["H"] * c["W"] == 1
            continue
        planted_cases += 1
        H, W = c["H"], c["W"]
        k = [w * H + h for (_, h, w) in inp["planted"]]
        t = tar[0, k]
        kept = (t[:, 0] >= 0).tolist()
        # order of geom_bounds._stage3_plants: c = 0 | +inf | -inf | tx = 0 | tx = H-1 | tx just above 0 | just below H-1 | ty = W-1 |
        # just below W-1 | tx = 0.75 | NaN tx | NaN ty | NaN c | ty just above 0 | ty = 0
        want = [c["thr"] < 0.5, True, False, False, False, True, True, False, True, True, False, False, False, True, False]
        assert kept == want, (gb.case_name("stage3", c), kept)
        assert t[5].tolist()[0] == 0 and t[6].tolist()[0] == H - 2 and t[8].tolist()[1] == W - 2 and t[9].tolist()[0] == 0 and t[13].tolist()[1] == 0
        assert torch.equal(src[0, k][torch.tensor(kept)], torch.tensor([[w, h] for (_, h, w) in inp["planted"]])[torch.tensor(kept)])
    assert planted_cases == len(gb.CASES["stage3"]) - 3


def test_sweep_data_reaches_the_edges():
    """What the sweep promises about its inputs: non-binary masks with exact zeros, simvol columns of zeros and magnitudes inside
    [1e-3, 1e3], simvol_bwd `out` with +0, -0 and small positive normals, dense query_K really dense and conditioned as stated,
    projective rows with ww in [1, 2], gather lists with the three kinds of invalid entry, all indices in range, and the first- /
    last-chunk lists."""
    for c in gb.CASES["simvol"]:
        inp = gb.inputs("simvol", c)
        assert set(inp["mask"].unique().tolist()) == {0.0, 0.5, 1.0, 2.0}
        for k in ("src", "tar"):
            a = inp[k].abs()
            assert float(a[a > 0].min()) >= 1e-3 and float(a.max()) <= 1e3
        assert bool((inp["src"][0, :, 3, 5] == 0).all()) and bool((inp["tar"][-1, :, 9, 2] == 0).all())
        m16 = gb.model("simvol", inp)[1]
        assert 0.05 < float((m16 == 0).double().mean()) < 0.6            # exact zeros are asserted on a good share, not on everything
    for c in gb.CASES["simvol_bwd"]:
        o = gb.inputs("simvol_bwd", c)["out"]
        neg0 = (o == 0) & torch.signbit(o)
        assert bool(neg0.any()) and bool(((o == 0) & ~torch.signbit(o)).any()) and bool(((o > 0) & (o < 1e-20)).any())
    for c in gb.CASES["pose2d"]:
        inp = gb.inputs("pose2d", c)
        K = inp["query_K"].double()
        assert float(torch.linalg.det(K).abs().min()) >= 2e5 and float(torch.linalg.cond(K).max()) < 3e3
        if c["K"] == "dense":
            assert float(K.abs().min()) > 1e-4          # every entry far above its own rounding (u |K| ~ 3e-5 at the top)
        else:
            assert bool((K[:, 1, 0] == 0).all() and (K[:, 2, 0] == 0).all() and (K[:, 2, 1] == 0).all())
            assert bool((K[:, 0, 0] != K[:, 1, 1]).all())
        th = torch.atan2(inp["inplane"][:, 1], inp["inplane"][:, 0])
        if c["B"] >= 4:
            assert {int(q) for q in torch.floor(th / (torch.pi / 2)).tolist()} == {-2, -1, 0, 1}
        assert bool((inp["query_M"][:, 0, 1] == 0).all() and (inp["query_M"][:, 0, 0] == inp["query_M"][:, 1, 1]).all())
    for c in gb.CASES["init_corr"]:
        if c["projective"]:
            M = gb.inputs("init_corr", c)["pred_Ms"]
            assert bool((M[:, 2, :2] > 0).all()) and float((M[:, 2, 0] + M[:, 2, 1]).max()) * c["size"] <= 1.0
    seen = set()
    for c in gb.CASES["gather"]:
        idx = gb.inputs("gather", c)["idx"]
        x, y = idx[..., 0], idx[..., 1]
        ok = ((x == -1) | ((x >= 0) & (x < c["W"]))) & ((y == -1) | ((y >= 0) & (y < c["H"])))
        assert bool(ok.all())
        v = (x != -1) & (y != -1)
        assert v.sum(1).tolist()[:2] == [0, c["N"]]
        if c["N"] >= 63:
            assert bool(((x[0] == -1) & (y[0] != -1)).any()) and bool(((x[0] != -1) & (y[0] == -1)).any()) and bool(((x[0] == -1) & (y[0] == -1)).any())
            p = y[1] * c["W"] + x[1]
            assert bool((p[1:] <= p[:-1]).all()) and (c["N"] < 1000 or bool((p[1:] == p[:-1]).any()))
            assert 0 < int(v[2].sum()) < c["N"]
        if c["N"] > 1024 and c["kind"] == "last_chunk":
            assert not bool(v[2, :((c["N"] - 1) // 1024) * 1024].any())
            seen.add("last")
        if c["N"] > 1024 and c["kind"] == "first_chunk":
            assert not bool(v[2, 1024:].any())
            seen.add("first")
    assert seen == {"last", "first"}
