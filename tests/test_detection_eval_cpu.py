"""CPU: DETECTION SCORING without a GPU: the hand-worked answers through the numpy restatement (tests/detection_eval_oracle.py) and through
the package's own accumulate / summarize, argument validation through the ABI, bad records, and the closed form of the matching (what
pp_det_match computes) against the restatement's sequential scan."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detection_eval_oracle as eo  # noqa: E402

from picopose_amd import _lib  # noqa: E402
from picopose_amd import detection_eval as de  # noqa: E402  (absent before the feature: every test here fails without it)

H, W = 24, 20
A_MASK = eo.rect(H, W, 2, 10, 3, 9)                  # 48 pixels
FAR = eo.rect(H, W, 14, 22, 11, 17)                  # disjoint from A_MASK


def _both(dets, anns, **kw):
    """The oracle's tables, accumulated and summarised by the oracle AND by the package: the two must agree, and the pair is returned."""
    m = eo.match(dets, anns, **kw)
    acc_o, acc = eo.accumulate(m), de.accumulate(m)
    assert np.array_equal(acc_o["precision"], acc["precision"]) and np.array_equal(acc_o["recall"], acc["recall"])
    s_o, s = eo.summarize(acc_o), de.summarize(acc)
    assert set(s) == set(eo.NAMES) | {"per_object_AP"} and s["per_object_AP"].keys() == s_o["per_object_AP"].keys()
    for k in eo.NAMES:
        assert abs(s[k] - s_o[k]) <= 1e-12, k
    return m, acc, s


def test_one_identical_detection_scores_one():
    m, acc, s = _both([eo.det(A_MASK, 0.9)], [eo.ann(A_MASK)])
    assert acc["precision"].shape == (10, 101, 1, 4, 3) and acc["recall"].shape == (10, 1, 4, 3)
    for k in eo.NAMES:
        assert abs(s[k] - 1) <= 1e-12 or s[k] == -1, (k, s[k])
    assert s["APm"] == -1 and s["APl"] == -1 and s["ARl"] == -1 and abs(s["APs"] - 1) <= 1e-12      # 48 pixels: COCO's "small" only
    assert abs(s["AP"] - 1) <= 1e-12 and abs(s["AR1"] - 1) <= 1e-12 and s["per_object_AP"].keys() == {1}
    for t in ("bbox",):
        assert abs(eo.score([eo.det(A_MASK, 0.9)], [eo.ann(A_MASK)], iou_type=t)["AP"] - 1) <= 1e-12


def test_false_positive_ahead_of_the_true_positive_halves_precision():
    m, acc, s = _both([eo.det(A_MASK, 0.5), eo.det(FAR, 0.9)], [eo.ann(A_MASK)])
    assert m["det_index"].tolist() == [1, 0] and m["dt_match"][0, 0].tolist() == [-1, 0]
    half = 1 / (2 + np.spacing(1))
    assert np.all(acc["precision"][:, :, 0, 0, 2] == half) and abs(half - 0.5) < 1e-15
    assert abs(s["AP50"] - 0.5) <= 1e-12 and abs(s["AP"] - 0.5) <= 1e-12
    assert s["AR1"] == 0 and s["AR10"] == 1                     # the one detection AR1 sees is the false positive


def test_second_detection_on_one_ground_truth_is_a_false_positive_unless_it_is_a_crowd():
    dets = [eo.det(A_MASK, 0.9), eo.det(A_MASK, 0.8)]
    m, acc, s = _both(dets, [eo.ann(A_MASK)])
    assert m["dt_match"][0, :, :].tolist() == [[0, -1]] * 10 and not m["dt_ignore"][:2].any() and m["gt_match"][0, 0].tolist() == [0]
    assert acc["precision"][0, 0, 0, 0, 2] == 1 / (1 + np.spacing(1)) and s["AR100"] == 1
    # a crowd: both match, both are ignored, and with nothing else in the category nothing is scored
    m, acc, s = _both(dets, [eo.ann(A_MASK, iscrowd=True)])
    assert m["dt_match"][0, 0].tolist() == [0, 0] and m["dt_ignore"][0].all() and m["gt_match"][0, 0].tolist() == [1] and m["gt_ignore"].all()
    assert np.all(acc["precision"] == -1) and s["AP"] == -1
    # ... and next to a plain ground truth the two count as neither true nor false positives
    m, acc, s = _both(dets + [eo.det(FAR, 0.7)], [eo.ann(A_MASK, iscrowd=True), eo.ann(FAR)])
    assert m["dt_match"][0, 0].tolist() == [0, 0, 1] and m["dt_ignore"][0, 0].tolist() == [1, 1, 0] and abs(s["AP"] - 1) <= 1e-12


def test_a_detection_on_an_ignored_ground_truth_counts_as_neither():
    m, acc, s = _both([eo.det(A_MASK, 0.9), eo.det(FAR, 0.8)], [eo.ann(A_MASK, ignore=True), eo.ann(FAR)])
    assert m["dt_match"][0, 0].tolist() == [0, 1] and m["dt_ignore"][0, 0].tolist() == [1, 0] and m["gt_ignore"][0].tolist() == [1, 0]
    assert abs(s["AP"] - 1) <= 1e-12 and s["AR100"] == 1          # one ground truth counts, one true positive, no false positive
    # the ignored one is tried only when no other qualifies: a detection over both takes the plain one
    m = eo.match([eo.det(A_MASK, 0.9)], [eo.ann(A_MASK, ignore=True), eo.ann(A_MASK)])
    assert m["dt_match"][0, 0].tolist() == [1] and not m["dt_ignore"][:2].any()


def test_no_detections_recall_zero_and_no_ground_truth_left_out():
    m, acc, s = _both([], [eo.ann(A_MASK)])
    assert np.all(acc["recall"][:, 0, 0, :] == 0) and np.all(acc["precision"][:, :, 0, 0, :] == 0) and s["AR100"] == 0 and s["AP"] == 0
    # category 2 has detections only: its cells stay -1 and the means leave them out
    m, acc, s = _both([eo.det(A_MASK, 0.9), eo.det(FAR, 0.8, cat=2)], [eo.ann(A_MASK)])
    assert m["categories"] == [1, 2] and np.all(acc["precision"][:, :, 1] == -1) and np.all(acc["recall"][:, 1] == -1)
    assert abs(s["AP"] - 1) <= 1e-12 and s["per_object_AP"][2] == -1 and abs(s["per_object_AP"][1] - 1) <= 1e-12
    # class-agnostic: one category 0, and the category-2 detection is now a false positive after the true one
    m, acc, s = _both([eo.det(A_MASK, 0.9), eo.det(FAR, 0.8, cat=2)], [eo.ann(A_MASK)], class_agnostic=True)
    assert m["categories"] == [0] and abs(s["AP"] - 1) <= 1e-12 and m["dt_match"][0, 0].tolist() == [0, -1]


def test_thresholds_are_met_exactly():
    dets, anns = eo.threshold_case()
    m = eo.match(dets, anns)
    assert m["inter"].reshape(5, 5)[0, 0] == 8 and m["iou"].reshape(5, 5)[0, 0] == 0.5 and m["iou"].reshape(5, 5)[1, 1] == 0.75
    assert m["iou_thrs"][0] == 0.5 and m["iou_thrs"][5] == 0.75
    assert m["dt_match"][0, :, 0].tolist() == [0] + [-1] * 9 and m["dt_match"][0, :, 1].tolist() == [1] * 6 + [-1] * 4
    assert m["dt_match"][0, 0].tolist() == [0, 1, 2, 2, 4] and m["gt_match"][0, 0].tolist() == [0, 1, 3, -1, 4]      # crowd twice; the LAST twin


def test_closed_form_equals_the_sequential_scan():
    dets, anns = eo.random_case(0)
    for kw in ({"area_ranges": eo.SMALL_RANGES}, {"iou_type": "bbox", "area_ranges": eo.SMALL_RANGES, "iou_thrs": [0.3, 0.5, 1.0]}):
        seq = eo.match(list(dets), list(anns), **kw)
        closed = eo.match(list(dets), list(anns), match_group=eo.match_group_closed, **kw)
        for k in eo.TABLES[2:]:
            assert np.array_equal(seq[k], closed[k]), k
        assert (seq["dt_match"] >= 0).any() and seq["dt_ignore"].any() and (seq["gt_ignore"].sum(axis=1) > 0).all()
    ng = seq["group_gt"][:, 1].tolist()
    assert {0, 1, 3, 64, 65, 130} <= set(ng) and {0, 1, 7, 100} <= set(seq["group_det"][:, 1].tolist())


def test_argument_validation_needs_no_gpu():
    L = _lib.lib()
    c = ctypes
    buf = (c.c_char * 256)()
    p = c.addressof(buf)
    arr = lambda v, t: (t * len(v))(*v)      # noqa: E731
    g1 = arr([0, 2, 0, 3, 0], c.c_int)
    tl = arr([0, 0, 0], c.c_int)

    def ov(bits=p, area=p, words=15, boxes=None, n_det=2, n_gt=3, groups=p, gh=g1, n_groups=1, tiles=p, th=tl, n_tiles=1, flags=p, n_pairs=6,
           inter=p, iou=p):
        return L.pp_det_overlaps(bits, area, words, boxes, n_det, n_gt, groups, gh, n_groups, tiles, th, n_tiles, flags, n_pairs, inter, iou, None)

    assert ov(bits=None) == -1 and ov(boxes=p) == -1 and ov(area=None) == -1 and ov(inter=None) == -1 and ov(words=0) == -1      # segm xor bbox
    assert ov(groups=None) == -1 and ov(gh=None) == -1 and ov(flags=None) == -1 and ov(iou=None) == -1 and ov(tiles=None) == -1 and ov(th=None) == -1
    assert ov(n_det=-1) == -1 and ov(n_gt=-1) == -1 and ov(n_groups=0) == -1 and ov(n_tiles=-1) == -1 and ov(n_pairs=-1) == -1
    assert ov(n_pairs=5) == -1 and ov(n_det=1) == -1 and ov(n_gt=2) == -1                                  # the block or a range leaves the call
    for bad in ([-1, 2, 0, 3, 0], [0, -2, 0, 3, 0], [0, 2, 1, 3, 0], [0, 2, 0, 3, 1], [0, 2, 0, 3, -1]):
        assert ov(gh=arr(bad, c.c_int)) == -1, bad
    for bad in ([1, 0, 0], [-1, 0, 0], [0, 8, 0], [0, 0, 8], [0, 4, 0], [0, -8, 0]):
        assert ov(th=arr(bad, c.c_int)) == -1, bad
    assert ov(n_tiles=0, tiles=None, th=None) == 0                                                         # nothing to do: PP_OK, no launch
    assert ov(gh=arr([0, 2, 0, 0, 0], c.c_int), n_tiles=0, n_pairs=0) == 0                                 # an empty side is legal

    r1, t1 = arr([0.0, 1e10], c.c_double), arr([0.5, 1.0], c.c_double)

    def mt(iou=p, n_pairs=6, groups=p, gh=g1, n_groups=1, n_det=2, n_gt=3, da=p, ga=p, flags=p, ranges=p, rh=r1, A=1, thrs=p, th=t1, T=2,
           dtm=p, dti=p, gtm=p, gti=p):
        return L.pp_det_match(iou, n_pairs, groups, gh, n_groups, n_det, n_gt, da, ga, flags, ranges, rh, A, thrs, th, T, dtm, dti, gtm, gti, None)

    for name in ("iou", "groups", "gh", "da", "ga", "flags", "ranges", "rh", "thrs", "th", "dtm", "dti", "gtm", "gti"):
        assert mt(**{name: None}) == -1, name
    assert mt(A=0) == -1 and mt(T=0) == -1 and mt(n_groups=0) == -1 and mt(n_det=-1) == -1 and mt(n_gt=-1) == -1 and mt(n_pairs=-1) == -1
    for bad in ([0.0, 0.5], [0.5, 1.5], [-0.1, 0.5], [float("nan"), 0.5]):
        assert mt(th=arr(bad, c.c_double)) == -1, bad
    assert mt(rh=arr([2.0, 1.0], c.c_double)) == -1 and mt(rh=arr([float("nan"), 1.0], c.c_double)) == -1
    assert mt(n_pairs=5) == -1 and mt(gh=arr([0, 2, 0, 4, 0], c.c_int)) == -1 and mt(gh=arr([1, 2, 0, 3, 0], c.c_int)) == -1
    assert mt(gh=arr([0, 1, 0, 4097, 0], c.c_int), n_det=1, n_gt=4097, n_pairs=4097) == -1                 # G_g > PP_DET_MAX_GT
    assert {"pp_det_overlaps", "pp_det_match"} <= set(_lib.declared_symbols())


def test_bad_records_are_named(tmp_path):
    good = eo.det(A_MASK, 0.9)
    assert de.read_detections([good]) == [good]
    path = tmp_path / "dets.json"
    path.write_text(json.dumps([good, eo.det(FAR, 0.5, compressed=True)]))
    assert len(de.read_detections(str(path))) == 2 and de.read_detections(path)[0] == good
    with pytest.raises(ValueError, match="list"):
        de.read_detections({"a": 1})
    for key in ("scene_id", "image_id", "category_id", "bbox", "score", "segmentation"):
        bad = {k: v for k, v in good.items() if k != key}
        with pytest.raises(ValueError, match="detection 1"):
            de.read_detections([good, bad])
    for key, value in (("bbox", [1, 2, 3]), ("bbox", [0, 0, -1, 2]), ("score", float("nan")), ("score", "high"), ("scene_id", 1.5), ("segmentation", [1, 2])):
        with pytest.raises(ValueError, match="detection 0"):
            de.read_detections([dict(good, **{key: value})])
    # match_detections: the checks run before the device is needed
    ann = eo.ann(A_MASK)
    with pytest.raises(ValueError, match="detection 1: no 'score'"):
        de.match_detections([good, {k: v for k, v in good.items() if k != "score"}], [ann])
    with pytest.raises(ValueError, match="annotation 0: no 'segmentation'"):
        de.match_detections([good], [{k: v for k, v in ann.items() if k != "segmentation"}], iou_type="bbox")
    with pytest.raises(ValueError, match=r"annotation 1: mask size \(37, 29\) is not the frame's \(24, 20\)"):
        de.match_detections([good], [ann, eo.ann(eo.rect(37, 29, 0, 4, 0, 4))])
    with pytest.raises(ValueError, match="detection 0: run lengths sum to"):
        de.match_detections([dict(good, segmentation={"size": [H, W], "counts": [5, 5]})], [ann])
    for kw in ({"iou_type": "keypoints"}, {"iou_thrs": [0.0]}, {"iou_thrs": [1.5]}, {"iou_thrs": []}, {"area_ranges": [[5, 1]]}, {"max_dets": (0,)},
               {"max_dets": 100}, {"workspace_bytes": 0}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            de.match_detections([good], [ann], **kw)
    # gt_annotations: the masks must be there, one id per mask
    with pytest.raises(ValueError, match="masks="):
        de.gt_annotations([1], {"visib_fract": np.ones(1)}, 1, 1)
    res = {"mask_visib": np.stack([A_MASK * 255, FAR * 0, FAR * 255]), "bbox_visib": np.array([[3, 2, 8, 9], [0, 0, -1, -1], [11, 14, 16, 21]]),
           "px_count_visib": np.array([48, 0, 48]), "visib_fract": np.array([1.0, 0.0, 0.05])}
    with pytest.raises(ValueError, match="2 obj_ids for 3 masks"):
        de.gt_annotations([1, 2], res, 1, 1)
    anns = de.gt_annotations([4, 5, 6], res, 3, 9)
    assert [(a["category_id"], a["ignore"], a["iscrowd"], a["bbox"]) for a in anns] == [(4, False, False, [3, 2, 6, 8]), (6, True, False, [11, 14, 6, 8])]
    assert anns[0]["segmentation"] == eo.ann(A_MASK)["segmentation"] and (anns[0]["scene_id"], anns[0]["image_id"]) == (3, 9)
