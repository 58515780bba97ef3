"""CPU: the appearance score's argument checks (no device is touched before they return), the oracle on the planted and random sets
the GPU tests use, the patch-validity rule on hand-made masks, and the combined-score ordering rule."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import appearance_oracle as ao  # noqa: E402
import proposal_oracle as po  # noqa: E402

from picopose_amd import _lib  # noqa: E402

EINVAL = -1


def _host_ptr(nbytes=256, misalign=0):
    buf = (ctypes.c_char * (nbytes + 32))()
    p = ctypes.addressof(buf)
    return buf, p + (-p) % 16 + misalign


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_appearance_match_rejects_bad_arguments_without_a_device():
    L = _lib.lib()
    keep, p = _host_ptr()
    good = dict(query=p, q_valid=p, P=3, bank=p, t_valid=p, R=4, pair_row=p, pair_row_host=_ints(2, 0, 2), N=16, C=8, patch_sim=p,
                patch_arg=p, n_valid=p, app=p)
    order = ("query", "q_valid", "P", "bank", "t_valid", "R", "pair_row", "pair_row_host", "N", "C", "patch_sim", "patch_arg", "n_valid", "app")
    call = lambda **kw: L.pp_appearance_match(*[{**good, **kw}[k] for k in order], None)  # noqa: E731
    for name in ("query", "q_valid", "bank", "t_valid", "pair_row", "pair_row_host", "patch_sim", "patch_arg", "n_valid", "app"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("P", "R", "N", "C"):
        for bad in (0, -1):
            assert call(**{name: bad}) == EINVAL, (name, bad)
    assert _lib.PP_APP_MAX_N >= 1024 and call(N=_lib.PP_APP_MAX_N + 1) == EINVAL
    assert call(C=6) == EINVAL                                   # not a multiple of 4
    assert call(C=_lib.PP_MATCH_MAX_C + 4) == EINVAL
    assert call(query=p + 4) == EINVAL and call(bank=p + 8) == EINVAL      # 16-byte loads
    assert call(pair_row_host=_ints(2, 4, 2)) == EINVAL          # past the bank
    assert call(pair_row_host=_ints(2, 0, -1)) == EINVAL
    assert call(R=2) == EINVAL                                   # the same rows against a smaller bank
    del keep


def test_patch_valid_rejects_bad_arguments_without_a_device():
    L = _lib.lib()
    keep, p = _host_ptr()
    assert L.pp_patch_valid(None, 2, 28, 14, p, p, None) == EINVAL
    assert L.pp_patch_valid(p, 2, 28, 14, None, p, None) == EINVAL
    assert L.pp_patch_valid(p, 2, 28, 14, p, None, None) == EINVAL
    for n, S, patch in ((0, 28, 14), (-1, 28, 14), (2, 0, 14), (2, -28, 14), (2, 28, 0), (2, 28, -14), (2, 30, 14), (2, 28, 56),
                        (2, _lib.PP_APP_MAX_S + 14, 14)):
        assert L.pp_patch_valid(p, n, S, patch, p, p, None) == EINVAL, (n, S, patch)
    del keep


def test_label_proposals_needs_a_bank_with_patches_before_touching_the_device():
    import torch

    from picopose_amd import proposals as pr

    bank = pr.DescriptorBank(torch.zeros(2, 8), [0, 1, 2], [5, 9])          # host tensors: nothing here may reach the device
    assert bank.patch_rows is None and bank.patch_valid is None
    with pytest.raises(ValueError, match="patches=True"):
        pr.label_proposals(None, None, [], bank, scene_id=1, img_id=1, appearance=True)
    with pytest.raises(ValueError, match="patches=True"):
        pr.appearance_scores(torch.zeros(1, 4, 8), torch.zeros(1, 4, dtype=torch.uint8), bank, [0])
    with pytest.raises(ValueError, match="together"):
        pr.DescriptorBank(torch.zeros(2, 8), [0, 1, 2], [5, 9], patch_rows=torch.zeros(2, 4, 8))
    with pytest.raises(ValueError, match="tem_mask"):
        pr.describe_templates(None, {"tem_rgb": torch.zeros(2, 3, 3, 28, 28)}, [5, 9], patches=True)
    full = pr.DescriptorBank(torch.zeros(2, 8), [0, 1, 2], [5, 9], torch.zeros(2, 4, 8), torch.zeros(2, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="one GPU"):             # host tensors never reach the entry as pointers
        pr.appearance_scores(torch.zeros(1, 4, 8), torch.zeros(1, 4, dtype=torch.uint8), full, [0])
    with pytest.raises(ValueError, match="appearance_weight"):
        pr.label_proposals(None, None, [], full, scene_id=1, img_id=1, appearance=True, appearance_weight=-1.0)


def test_pipeline_passes_the_appearance_keywords_to_the_labelling():
    from picopose_amd import pipeline

    assert "appearance" in pipeline.LABEL_KEYS and "appearance_weight" in pipeline.LABEL_KEYS


def test_error_bounds_are_the_stated_formulas():
    u = 2.0 ** -24
    for C in ao.C_SET:
        g = C * u / (1 - C * u)
        e = 2 * g + 8 * u
        assert ao.e_cos(C) == pytest.approx(e, rel=1e-12) and ao.sim_bound(C) == pytest.approx(1.01 * e, rel=1e-12)
        for n in (1, 65, 1024):
            gn = n * u / (1 - n * u)
            assert ao.app_bound(C, n) == pytest.approx(1.01 * (e + gn * (1 + e) + u), rel=1e-12)
    assert ao.e_cos(1024) < po.err_bound(1024) and ao.app_bound(1024, 1024) < 2e-4


@pytest.mark.parametrize("C", ao.PLANTED_C)
@pytest.mark.parametrize("N", ao.PLANTED_N)
def test_oracle_recovers_the_planted_patches(N, C):
    for P in (3, 5):
        q, qv, bank, tv, rows, perm = ao.planted_case(P, N, C)
        assert all(tv[r][perm[p]].all() for p, r in enumerate(rows))           # planted on valid template patches only
        m = ao.appearance(q, qv, bank, tv, rows)
        assert np.array_equal(m["patch_arg"], perm) and ao.undecided(m, C) == 0   # no planted case may be left out
        assert (m["app"] > 0.9).all() and m["patch_sim"].max() <= 1 + 1e-12
        assert np.array_equal(m["n_valid"], qv.sum(1))


@pytest.mark.parametrize("C", ao.C_SET)
@pytest.mark.parametrize("N", ao.N_SET)
def test_the_seed_stays_inside_the_cap(N, C):
    for P in ao.P_SET:
        for pattern in ao.PATTERNS:
            q, qv, bank, tv, rows = ao.random_case(P, N, C, pattern)
            assert sorted(rows.tolist()) != rows.tolist() or P == 1
            assert P == 1 or len(set(rows.tolist())) < P                        # one view is used twice
            m = ao.appearance(q, qv, bank, tv, rows)
            assert ao.undecided(m, C) <= ao.UNDECIDED_CAP * P * N, (P, pattern, ao.undecided(m, C))
            if pattern == "no_template":
                assert (m["patch_sim"] == 0).all() and (m["patch_arg"] == -1).all() and (m["app"] == 0).all()
            if pattern == "no_query":
                assert (m["n_valid"] == 0).all() and (m["app"] == 0).all() and (m["patch_arg"] >= 0).all()
            if pattern == "one":
                assert (m["n_valid"] == 1).all() and all((m["patch_arg"][p] == np.nonzero(tv[r])[0][0]).all() for p, r in enumerate(rows))


def test_oracle_takes_the_lowest_index_among_equal_maxima_and_skips_invalid_patches():
    rng = np.random.default_rng(5)
    bank = rng.standard_normal((1, 8, 16)).astype(np.float32)
    bank[0, 7] = bank[0, 3]
    bank[0, 1] = bank[0, 3]                                       # ... a third copy, which is not valid
    tv = np.ones((1, 8), np.uint8)
    tv[0, 1] = 0
    q = np.repeat(bank[:, 3:4], 8, axis=1)
    m = ao.appearance(q, np.ones((1, 8), np.uint8), bank, tv, [0])
    assert (m["patch_arg"] == 3).all() and (m["margin"] == 0).all() and m["app"][0] == pytest.approx(1.0, abs=1e-12)


def test_patch_valid_of_hand_made_masks():
    p, S = 14, 28
    mask = np.zeros((3, S, S), np.float32)
    mask[0, :7, :14] = 1.0                                       # patch 0: 98 of 196 pixels, exactly half: valid
    mask[0, 14:21, 14:28] = 1.0                                  # patch 3: the same, one pixel short: not valid
    mask[0, 14, 14] = 0.0
    mask[1, :14, 14:] = 0.75                                     # patch 1 (py 0, px 1): the token order is row-major
    mask[1, 14:, :14] = 0.5                                      # patch 2: 0.5 is not above 0.5
    mask[2] = np.nan                                             # a NaN is not counted
    mask[2, 14:, 14:] = 1.0
    valid, n = ao.patch_valid(mask, p)
    assert valid.dtype == np.uint8 and valid.tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]] and n.tolist() == [1, 1, 1]
    big = np.zeros((1, 224, 224), np.float32)
    big[0, 100:, :] = 1.0                                        # row 7 of the 16 x 16 grid has 12 of its 14 pixel rows set
    valid, n = ao.patch_valid(big, 14)
    assert n[0] == 16 * 9 and valid[0].reshape(16, 16)[7].all() and not valid[0].reshape(16, 16)[6].any()


def test_combined_score_and_ordering_rule_on_a_hand_made_table():
    from picopose_amd.proposals import combined_scores, nms_masks

    sem = np.float32([0.75, 0.5, 0.625, 0.9, 0.25])
    app = np.float32([0.25, 0.5, 0.375, 0.5, 1.0])
    for w, want in ((1.0, [0.5, 0.5, 0.5, 0.7, 0.625]), (0.0, sem.astype(np.float64).tolist()), (3.0, [0.375, 0.5, 0.4375, 0.6, 0.8125])):
        got = combined_scores(sem, app, w)
        assert got.dtype == np.float64 and np.allclose(got, want, atol=1e-7) and np.array_equal(got, ao.combine(sem, app, w))
    score = combined_scores(sem, app, 1.0)
    assert score[0] == score[1] == score[2] == 0.5               # dyadic values: the tie is exact in float64
    inter = np.diag([10] * 5).astype(np.int32)
    labels, area = np.zeros(5, np.int32), np.int32([10] * 5)
    # no overlaps: the visiting order itself, descending combined score, lower index first among equals
    assert nms_masks(score, labels, inter, area, 0.25) == po.nms(score, labels, inter, area, 0.25) == [3, 4, 0, 1, 2]
    inter[0, 1] = inter[1, 0] = 9                                # 0 and 1 overlap and tie: the lower index survives
    inter[2, 4] = inter[4, 2] = 9                                # 4 beats 2
    assert nms_masks(score, labels, inter, area, 0.25) == po.nms(score, labels, inter, area, 0.25) == [3, 4, 0]
    # the semantic order (0.9, 0.75, 0.625, ...) would have visited 0 before 4 and 2 before 1
    assert nms_masks(sem, labels, inter, area, 0.25) == [3, 0, 2]
