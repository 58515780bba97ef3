"""CPU: picopose_amd/scoring.py, the host core of the two detection scorers, on cases small enough to state by hand: the
precision-recall curve of one cell and the group plan with its two errors.  (The scorers' own CPU tests hold both against the numpy
restatements under tests/; those stay independent of this module.)"""
import numpy as np
import pytest

from picopose_amd import scoring


def test_pr_curve_by_hand():
    # a false positive ahead of the true positive, one ground truth: rc = [0, 1], pr = [0, 1 / 2] -> 1 / 2 from the right
    matched, ignored = np.array([[False, True]]), np.zeros((1, 2), bool)
    p, r = scoring.pr_curve(matched, ignored, 1)
    assert p.shape == (1, 101) and p.dtype == np.float64 and r.shape == (1,)
    assert r[0] == 1.0 and np.all(p[0] == 1 / (2 + np.spacing(1))) and abs(p[0, 0] - 0.5) < 1e-15
    # an ignored record, matched or not, wherever it stands, moves nothing
    for pos in range(3):
        for hit in (False, True):
            m, ig = np.insert(matched, pos, hit, axis=1), np.insert(ignored, pos, True, axis=1)
            p2, r2 = scoring.pr_curve(m, ig, 1)
            assert p2.tobytes() == p.tobytes() and r2.tobytes() == r.tobytes()
    # two ground truths, only one found: the samples above recall 1 / 2 are 0; the rows (thresholds) are independent
    p, r = scoring.pr_curve(np.array([[True, False], [False, False]]), np.zeros((2, 2), bool), 2)
    assert r.tolist() == [0.5, 0.0] and np.all(p[0, :51] == 1 / (1 + np.spacing(1))) and not p[0, 51:].any()
    assert np.all(p[1, 0] == 0) and not p[1, 1:].any()
    # no record: recall 0, a precision of zeros
    p, r = scoring.pr_curve(np.zeros((3, 0), bool), np.zeros((3, 0), bool), 4)
    assert p.shape == (3, 101) and not p.any() and r.tolist() == [0.0, 0.0, 0.0]
    assert scoring.mean_valid(np.array([-1.0, 0.25, 0.75])) == 0.5 and scoring.mean_valid(np.array([-1.0])) == -1.0


def _rows(*lists):
    return [np.array(x, np.int64) for x in lists]


def test_group_plan_by_hand():
    keys = [((1, 1), 5), ((1, 1), 6), ((1, 2), 5)]
    # group 0: 2 x 3, group 1: no ground truth, group 2: nothing scored
    scored, truth, pair, scored_index, truth_index, n_pairs = plan = scoring.plan_groups(
        keys, _rows([7, 2], [4, 9, 0], []), _rows([3, 1, 8], [], [5, 6]), 4096, "object", "ground truths")
    assert scored.tolist() == [[0, 2], [2, 3], [5, 0]] and truth.tolist() == [[0, 3], [3, 0], [3, 2]]
    assert pair.tolist() == [0, 6, 6] and n_pairs == 6
    assert scored_index.tolist() == [7, 2, 4, 9, 0] and truth_index.tolist() == [3, 1, 8, 5, 6]
    assert all(a.dtype == np.int64 for a in plan[:5])
    assert scoring.first(np.array([2, 0, 3])).tolist() == [0, 2, 2]
    rows = scoring.group_rows(scored, truth, pair)
    assert rows.dtype == np.int32 and rows.flags["C_CONTIGUOUS"] and rows.tolist() == [[0, 2, 0, 3, 0], [2, 3, 3, 0, 6], [5, 0, 3, 2, 6]]
    # three groups with pairs: 2 x 3, 1 x 2, 4 x 1 -> offsets 0, 6, 8 and 12 pairs
    plan = scoring.plan_groups(keys, _rows([0, 1], [2], [3, 4, 5, 6]), _rows([0, 1, 2], [3, 4], [5]), 4096, "category", "annotations")
    assert plan[2].tolist() == [0, 6, 8] and plan[5] == 12
    # no group at all
    scored, truth, pair, scored_index, _, n_pairs = scoring.plan_groups([], [], [], 4096, "object", "ground truths")
    assert scored.shape == (0, 2) and truth.shape == (0, 2) and pair.shape == (0,) and n_pairs == 0
    assert scored_index.dtype == np.int64 and scoring.group_rows(scored, truth, pair).shape == (0, 5)


def test_group_plan_errors_carry_the_callers_nouns():
    keys = [((1, 1), 5), ((1, 2), 7)]
    for kind, noun in (("object", "ground truths"), ("category", "annotations")):
        with pytest.raises(ValueError, match=rf"image \(1, 2\), {kind} 7: 5 {noun}, more than the 4 of one group"):
            scoring.plan_groups(keys, _rows([0] * 9, []), _rows([0], [1, 2, 3, 4, 5]), 4, kind, noun)
    # the scored side has no bound of its own here; one side alone (pose_nms' estimates) has
    assert scoring.plan_groups(keys, _rows([0] * 9, []), _rows([0], [1]), 4, "object", "ground truths")[5] == 9
    with pytest.raises(ValueError, match=r"image \(1, 1\), object 5: 9 estimates, more than the 4 of one group"):
        scoring.axis(keys, _rows([0] * 9, []), 4, "object", "estimates")
    table, index = scoring.axis(keys, _rows([0] * 9, []), None, "object", "estimates")
    assert table.tolist() == [[0, 9], [9, 0]] and index.tolist() == [0] * 9
    # 2^19 scored rows against 4096 ground truths: 2^31 pairs, which 32-bit block offsets do not hold; the plan counts them and the
    # caller holds the call's count, or each chunk's, to the guard
    n_pairs = scoring.plan_groups(keys[:1], [np.zeros(2 ** 19, np.int64)], [np.zeros(4096, np.int64)], 4096, "object", "ground truths")[5]
    assert n_pairs == 2 ** 31
    for where in ("call", "chunk"):
        with pytest.raises(ValueError, match=f"{2 ** 31} pairs in one {where}: more than 32-bit block offsets hold"):
            scoring.check_offsets(n_pairs, where)
        scoring.check_offsets(n_pairs - 1, where)
    with pytest.raises(ValueError, match="7 pairs in one call: more than 32-bit block offsets hold"):      # (the records of a side count too)
        scoring.check_offsets(7, "call", 2 ** 31)
