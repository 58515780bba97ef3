"""CPU: 6D DETECTION SCORING without a GPU: the hand-worked answers through the numpy restatement (tests/pose_detection_oracle.py) and
through the package's own accumulate / summarize, the planning (images filter, per-image cut, empty sides, gt_info forms) against the
restatement, argument validation of both entries through the ABI, and the ValueErrors of the Python layer."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_detection_oracle as po  # noqa: E402

from picopose_amd import _lib  # noqa: E402
from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import pose_detection_eval as pe  # noqa: E402  (absent before the feature: every test here fails without it)

EYE = np.eye(3)


def _estimates(rows):
    """rows of (scene, im, obj, score) -> read_bop_results' dict with identity poses."""
    a = np.array(rows, dtype=np.float64).reshape(-1, 4)
    n = len(a)
    return {"scene_id": a[:, 0].astype(np.int64), "im_id": a[:, 1].astype(np.int64), "obj_id": a[:, 2].astype(np.int64), "score": a[:, 3].copy(),
            "R": np.tile(EYE, (n, 1, 1)), "t": np.zeros((n, 3)), "time": np.zeros(n)}


def _gt(obj_ids):
    n = len(obj_ids)
    return {"obj_id": np.array(obj_ids, np.int64), "R": np.tile(EYE, (n, 1, 1)), "t": np.zeros((n, 3))}


def _assert_plans_equal(a, b):
    for k in po.LAYOUT:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert a["images"] == b["images"] and a["objects"] == b["objects"] and a["n_pairs"] == b["n_pairs"]


def _both(plan, errors, limits):
    """The oracle's tables, accumulated and summarised by the oracle AND by the package: the two must agree."""
    m = dict(plan, metrics=("mssd", "mspd"), **po.match(plan, errors, limits))
    acc_o, acc = po.accumulate(m), pe.accumulate(m)
    assert acc_o["precision"].tobytes() == acc["precision"].tobytes() and acc_o["recall"].tobytes() == acc["recall"].tobytes()
    s_o, s = po.summarize(acc_o), pe.summarize(acc)
    for k in ("AP", "AP_MSSD", "AP_MSPD"):
        assert abs(s[k] - s_o[k]) <= 1e-12, k
    assert s["per_object"].keys() == s_o["per_object"].keys()
    for o in s_o["per_object"]:
        for k in ("AP", "AP_MSSD", "AP_MSPD"):
            assert abs(s["per_object"][o][k] - s_o["per_object"][o][k]) <= 1e-12, (o, k)
    return m, acc, s


def test_hit_miss_hit_by_hand():
    est = _estimates([(1, 1, 5, 0.9), (1, 1, 5, 0.8), (1, 1, 5, 0.7)])
    limits = np.full((1, 2, 10), 10.0)
    # two ground truths, neither ignored: the estimates hit, miss, hit at every threshold of both metrics
    ann = pe.pose_annotations({1: {1: _gt([5, 5])}})
    plan = pe.plan_groups(est, ann)
    _assert_plans_equal(plan, po.plan(est, po.annotations({1: {1: _gt([5, 5])}})))
    block = np.array([[1, 100], [100, 100], [100, 1]], np.float32).ravel()
    m, acc, s = _both(plan, np.stack([block, block]), limits)
    assert m["est_match"][0, 0].tolist() == [0, -1, 1] and not m["est_ignore"].any() and m["gt_match"][1, 9].tolist() == [0, 2]
    want = (51 + 50 * 2 / 3) / 101
    assert acc["precision"].shape == (2, 10, 101, 1) and np.all(acc["recall"] == 1)
    for k in ("AP", "AP_MSSD", "AP_MSPD"):
        assert abs(s[k] - want) <= 1e-12, (k, s[k])
    # the miss matched to an IGNORED third instance is neither a true nor a false positive
    info = {1: {"1": [{"visib_fract": 1.0}, {"visib_fract": 0.5}, {"visib_fract": 0.05}]}}
    ann3 = pe.pose_annotations({1: {1: _gt([5, 5, 5])}}, info)
    assert ann3["ignore"].tolist() == [False, False, True]
    plan3 = pe.plan_groups(est, ann3)
    block3 = np.array([[1, 100, 100], [100, 100, 1], [100, 1, 100]], np.float32).ravel()
    m, acc, s = _both(plan3, np.stack([block3, block3]), limits)
    assert m["est_match"][0, 0].tolist() == [0, 2, 1] and m["est_ignore"][1, 3].tolist() == [0, 1, 0]
    for k in ("AP", "AP_MSSD", "AP_MSPD"):
        assert abs(s[k] - 1) <= 1e-12, (k, s[k])
    # an object with only ignored ground truth is -1 and left out of the mean
    info2 = {1: {1: [{"visib_fract": 1.0}, {"visib_fract": 0.5}, {"visib_fract": 0.0}]}}
    ann4 = pe.pose_annotations({1: {1: _gt([5, 5, 6])}}, info2)
    est4 = _estimates([(1, 1, 5, 0.9), (1, 1, 5, 0.8), (1, 1, 5, 0.7), (1, 1, 6, 0.95)])
    plan4 = pe.plan_groups(est4, ann4)
    assert plan4["objects"] == [5, 6] and plan4["group_est"].tolist() == [[0, 3], [3, 1]] and plan4["group_pair"].tolist() == [0, 6]
    err4 = np.concatenate([block, np.array([100], np.float32)])
    m, acc, s = _both(plan4, np.stack([err4, err4]), np.full((2, 2, 10), 10.0))
    assert np.all(acc["precision"][..., 1] == -1) and np.all(acc["recall"][..., 1] == -1)
    assert s["per_object"][6] == {"AP_MSSD": -1.0, "AP_MSPD": -1.0, "AP": -1.0} and abs(s["AP"] - want) <= 1e-12
    assert abs(s["per_object"][5]["AP"] - want) <= 1e-12 and s["recall"]["mssd"].shape == (10, 2)


def test_the_strict_limit_equal_errors_and_the_ignored_class():
    est = _estimates([(1, 1, 5, 0.9), (1, 1, 5, 0.8)])
    ann = po.annotations({1: {1: _gt([5, 5, 5])}}, {1: {1: [{"visib_fract": 0.0}, {"visib_fract": 1.0}, {"visib_fract": 1.0}]}})
    plan = po.plan(est, ann)
    # estimate 0: the ignored instance 0 is nearest, instances 1 and 2 tie: the lowest non-ignored index wins; estimate 1: exactly at the
    # limit of instance 2 (no match at t = 0, a match at t = 1), the ignored one has +inf and a NaN stands where instance 1 was taken
    err = np.array([[0.5, 2, 2], [np.inf, np.nan, 4]], np.float32).ravel()[None]
    limits = np.array([4.0, np.nextafter(4.0, 5.0)]).reshape(1, 1, 2)
    m = po.match(plan, err, limits)
    assert m["est_match"][0].tolist() == [[1, -1], [1, 2]] and not m["est_ignore"].any() and m["gt_match"][0].tolist() == [[-1, 0, -1], [-1, 0, 1]]
    # only the ignored one qualifies: matched, and ignored; a negative zero never qualifies
    err = np.array([[0.5, 9, 9], [-0.0, 9, 9]], np.float32).ravel()[None]
    m = po.match(plan, err, limits)
    assert m["est_match"][0, 0].tolist() == [0, -1] and m["est_ignore"][0, 0].tolist() == [1, 0]


def test_planning_filter_cut_and_empty_sides(tmp_path):
    # image (1, 1): objects 5 and 6, four estimates with equal scores across the objects; image (1, 2): ground truth only; image (2, 1):
    # estimates only; image (2, 7): dropped by the filter
    est = _estimates([(1, 1, 6, 0.5), (1, 1, 5, 0.5), (1, 1, 5, 0.9), (1, 1, 6, 0.5), (2, 1, 5, 0.3), (2, 7, 5, 0.99), (1, 1, 5, 0.5)])
    gt = {1: {1: _gt([5, 6, 5]), 2: _gt([6])}, 2: {7: _gt([5])}}
    ann = pe.pose_annotations(gt)
    assert not ann["ignore"].any() and ann["inst"].tolist() == [0, 1, 2, 0, 0] and ann["scene_id"].tolist() == [1, 1, 1, 1, 2]
    path = tmp_path / "targets.json"
    path.write_text(json.dumps([{"scene_id": 1, "im_id": 1}, {"scene_id": 1, "im_id": 2}, {"scene_id": 2, "im_id": 1}, {"scene_id": 1, "im_id": 1}]))
    images = pe.read_image_targets(str(path))
    assert images == [(1, 1), (1, 2), (2, 1)]
    for cut in (None, 100, 3, 1):
        plan = pe.plan_groups(est, ann, images=images, max_per_image=cut)
        _assert_plans_equal(plan, po.plan(est, po.annotations(gt), images=images, max_per_image=cut))
    plan = pe.plan_groups(est, ann, images=images, max_per_image=3)
    # the cut keeps rows 2 (0.9), then 0 and 1 among the four at 0.5: the lower rows; object 6 keeps one estimate
    assert plan["images"] == [(1, 1), (1, 2), (2, 1)] and plan["objects"] == [5, 6]
    assert plan["est_index"].tolist() == [2, 1, 0, 4] and plan["group_est"].tolist() == [[0, 2], [2, 1], [3, 0], [3, 1]]
    assert plan["group_gt"].tolist() == [[0, 2], [2, 1], [3, 1], [4, 0]] and plan["gt_index"].tolist() == [0, 2, 1, 3]
    assert plan["group_pair"].tolist() == [0, 4, 5, 5] and plan["n_pairs"] == 5
    assert plan["pair_est"].tolist() == [2, 2, 1, 1, 0] and plan["pair_gt"].tolist() == [0, 2, 0, 2, 1]
    everything = pe.plan_groups(est, ann, max_per_image=None)
    assert everything["images"] == [(1, 1), (1, 2), (2, 1), (2, 7)] and everything["est_index"].tolist() == [2, 1, 6, 0, 3, 4, 5]
    # no record at all: no group, and the tables are empty without a device
    none = pe.plan_groups(_estimates([]), pe.pose_annotations({}))
    assert none["n_pairs"] == 0 and len(none["group_pair"]) == 0
    t = pe.match_pose_errors(none, np.zeros((2, 0), np.float32), np.zeros((0, 2, 10)))
    assert t["est_match"].shape == (2, 10, 0) and t["gt_match"].shape == (2, 10, 0)
    s = pe.summarize(pe.accumulate(dict(none, **t)))
    assert s["AP"] == -1 and s["per_object"] == {}


def test_gt_info_forms():
    gt = {3: {4: _gt([1, 2]), 9: _gt([1])}}
    fr = {4: [0.05, 0.1], 9: [0.0999]}
    ints = {3: {im: [{"visib_fract": f} for f in v] for im, v in fr.items()}}
    strs = json.loads(json.dumps({"3": {str(im): [{"visib_fract": f, "px_count_all": 7} for f in v] for im, v in fr.items()}}))
    for info in (ints, strs):
        assert pe.pose_annotations(gt, info)["ignore"].tolist() == [True, False, True]
    assert pe.pose_annotations(gt, ints, min_visib_fract=0.05)["ignore"].tolist() == [False, False, False]
    assert pe.pose_annotations(gt, ints)["ignore"].tolist() == po.annotations(gt, ints)["ignore"].tolist()
    with pytest.raises(ValueError, match="scene 3, image 9: 2 info entries for 1 instances"):
        pe.pose_annotations(gt, {3: {4: ints[3][4], 9: ints[3][4]}})
    with pytest.raises(ValueError, match="scene 3, image 9: no info"):
        pe.pose_annotations(gt, {3: {4: ints[3][4]}})
    with pytest.raises(ValueError, match="no scene 3"):
        pe.pose_annotations(gt, {})
    with pytest.raises(ValueError, match="instance 1: no 'visib_fract'"):
        pe.pose_annotations(gt, {3: {4: [{"visib_fract": 1}, {}], 9: ints[3][9]}})


def test_argument_validation_needs_no_gpu():
    L = _lib.lib()
    c = ctypes
    buf = (c.c_char * 256)()
    p = c.addressof(buf)
    arr = lambda v, t: (t * len(v))(*v)      # noqa: E731
    g1 = arr([0, 2, 0, 3, 0], c.c_int)
    l1 = arr([1.0] * 4, c.c_double)

    def mt(err=p, M=2, n_pairs=6, groups=p, gh=g1, n_groups=1, n_est=2, n_gt=3, ign=p, lim=p, lh=l1, T=2, em=p, ei=p, gm=p):
        return L.pp_pose_match(err, M, n_pairs, groups, gh, n_groups, n_est, n_gt, ign, lim, lh, T, em, ei, gm, None)

    for name in ("err", "groups", "gh", "ign", "lim", "lh", "em", "ei", "gm"):
        assert mt(**{name: None}) == -1, name
    assert mt(n_pairs=-1) == -1 and mt(n_est=-1) == -1 and mt(n_gt=-1) == -1 and mt(n_groups=0) == -1 and mt(M=0) == -1 and mt(T=0) == -1
    assert mt(M=5, lh=arr([1.0] * 10, c.c_double)) == -1 and mt(M=-1) == -1 and mt(T=-2) == -1                # M above PP_POSE_MAX_METRICS
    for bad in ([-1, 2, 0, 3, 0], [0, -2, 0, 3, 0], [0, 2, -1, 3, 0], [0, 2, 0, -3, 0], [0, 2, 0, 3, -1],     # a negative field
                [1, 2, 0, 3, 0], [0, 3, 0, 3, 0], [0, 2, 1, 3, 0], [0, 2, 0, 4, 0], [0, 2, 0, 3, 1]):         # a range or the block leaves the call
        assert mt(gh=arr(bad, c.c_int)) == -1, bad
    assert mt(n_pairs=5) == -1
    assert mt(gh=arr([0, 1, 0, 4097, 0], c.c_int), n_est=1, n_gt=4097, n_pairs=4097) == -1                      # G_g > PP_POSE_MAX_GROUP
    for k in range(4):
        bad = [1.0] * 4
        bad[k] = float("nan")
        assert mt(lh=arr(bad, c.c_double)) == -1, k

    n1 = arr([0, 3, 0], c.c_int)
    d1 = arr([5.0], c.c_double)

    def nm(dist=p, n_tri=3, groups=p, gh=n1, n_groups=1, n_est=3, lim=p, lh=d1, keep=p):
        return L.pp_pose_nms(dist, n_tri, groups, gh, n_groups, n_est, lim, lh, keep, None)

    for name in ("dist", "groups", "gh", "lim", "lh", "keep"):
        assert nm(**{name: None}) == -1, name
    assert nm(n_tri=-1) == -1 and nm(n_est=-1) == -1 and nm(n_groups=0) == -1 and nm(n_groups=-1) == -1
    for bad in ([-1, 3, 0], [0, -3, 0], [0, 3, -1], [1, 3, 0], [0, 4, 0], [0, 3, 1]):
        assert nm(gh=arr(bad, c.c_int)) == -1, bad
    assert nm(n_tri=2) == -1                                                                                  # the triangle leaves the call
    assert nm(gh=arr([0, 4097, 0], c.c_int), n_est=4097, n_tri=4097 * 2048) == -1                             # E_g > PP_POSE_MAX_GROUP
    assert nm(lh=arr([float("nan")], c.c_double)) == -1 and nm(lh=arr([-1.0], c.c_double)) == -1
    assert {"pp_pose_match", "pp_pose_nms"} <= set(_lib.declared_symbols())
    assert (_lib.PP_POSE_MAX_GROUP, _lib.PP_POSE_MAX_METRICS, _lib.PP_POSE_NMS_FIELDS) == (4096, 4, 3) == (pe.MAX_GROUP, pe.MAX_METRICS, 3)


def test_bad_arguments_are_named_before_any_device_work():
    est = _estimates([(1, 1, 5, 0.9), (1, 1, 5, 0.8)])
    ann = pe.pose_annotations({1: {1: _gt([5, 5, 5])}})
    plan = pe.plan_groups(est, ann)
    err, lim = np.zeros((2, 6), np.float32), np.ones((1, 2, 10))
    for bad_err, bad_lim, what in ((np.zeros((2, 5), np.float32), lim, "errors must be"), (np.zeros((2, 6)), lim, "errors must be"),
                                   (np.zeros((1, 6), np.float32), lim, "errors must be"), (err, np.ones((2, 2, 10)), "limits must be"),
                                   (err, np.ones((1, 2)), "limits must be"), (np.zeros((5, 6), np.float32), np.ones((1, 5, 10)), "M must be"),
                                   (err, np.where(np.arange(20).reshape(1, 2, 10) == 13, np.nan, 1.0), r"limits\[0, 1, 3\] is NaN")):
        with pytest.raises(ValueError, match=what):
            pe.match_pose_errors(plan, bad_err, bad_lim)
    with pytest.raises(ValueError, match="estimate 1: 'score' must be a finite number"):
        pe.plan_groups(dict(est, score=np.array([0.5, np.nan])), ann)
    with pytest.raises(ValueError, match="estimates: no 'score'"):
        pe.plan_groups({k: v for k, v in est.items() if k != "score"}, ann)
    with pytest.raises(ValueError, match="2 scene_ids for 1 im_ids"):
        pe.plan_groups(dict(est, im_id=np.array([1])), ann)
    for cut in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="max_per_image"):
            pe.plan_groups(est, ann, max_per_image=cut)
    with pytest.raises(ValueError, match="images must be"):
        pe.plan_groups(est, ann, images=[1, 2])
    with pytest.raises(ValueError, match="image target 1"):
        pe.read_image_targets([{"scene_id": 1, "im_id": 2}, {"scene_id": 1}])
    # a group above the cap, on either entry
    big = pe.pose_annotations({1: {1: _gt([5] * 4097)}})
    with pytest.raises(ValueError, match=r"image \(1, 1\), object 5: 4097 ground truths, more than the 4096"):
        pe.plan_groups(est, big)
    assert pe.plan_groups(est, pe.pose_annotations({1: {1: _gt([5] * 4096)}}))["n_pairs"] == 8192
    many = _estimates([(1, 1, 5, 0.5)] * 4097)
    with pytest.raises(ValueError, match=r"image \(1, 1\), object 5: 4097 estimates, more than the 4096"):
        pe.plan_nms(many)
    # the objects must be known to the models, the cameras must hold every image with pairs: all before the device is needed
    V = np.array([[x, y, z] for x in (-1.0, 1) for y in (-1.0, 1) for z in (-1.0, 1)], np.float32) * 40
    models = ev.ObjectModels({5: {"vertices": V, "info": {"diameter": 138.6}}}, device="cpu")
    cams = {1: {1: {"K": np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]), "depth_scale": 1.0}}}
    with pytest.raises(ValueError, match="estimate 1: unknown obj_id 6"):
        pe.match_poses(dict(est, obj_id=np.array([5, 6])), ann, models, cams)
    with pytest.raises(ValueError, match="annotation 2: unknown obj_id 8"):
        pe.match_poses(est, pe.pose_annotations({1: {1: _gt([5, 5, 8])}}), models, cams)
    with pytest.raises(ValueError, match="estimate 1: unknown obj_id 7"):
        pe.pose_nms(dict(est, obj_id=np.array([5, 7])), models)
    with pytest.raises(ValueError, match="cameras holds no entry for scene 1, image 1"):
        pe.match_poses(est, ann, models, {1: {2: cams[1][1]}})
    with pytest.raises(ValueError, match="one length"):
        pe.match_poses(est, ann, models, cams, thresholds_mssd=[0.1, 0.2])
    with pytest.raises(ValueError, match="thresholds_mspd"):
        pe.match_poses(est, ann, models, cams, thresholds_mssd=[0.1], thresholds_mspd=[-5.0])
    with pytest.raises(ValueError, match=r"R must be \(2, 3, 3\)"):
        pe.match_poses(dict(est, R=np.zeros((2, 9))), ann, models, cams)
    for d in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="nms_dist"):
            pe.pose_nms(est, models, nms_dist=d)
    nplan = pe.plan_nms(est)
    with pytest.raises(ValueError, match="dist must be"):
        pe.nms_walk(nplan, np.zeros(2, np.float32), np.ones(1))
    with pytest.raises(ValueError, match="limit must be"):
        pe.nms_walk(nplan, np.zeros(1, np.float32), np.array([-1.0]))


def test_nms_plan_and_walk_of_the_restatement():
    est = _estimates([(1, 1, 5, 0.5), (1, 1, 5, 0.9), (1, 1, 6, 0.1), (1, 1, 5, 0.5), (2, 1, 5, 0.4)])
    a, b = pe.plan_nms(est), po.plan_nms(est)
    for k in ("group_est", "group_tri", "group_obj", "est_index", "tri_early", "tri_late"):
        assert a[k].dtype == b[k].dtype and a[k].tolist() == b[k].tolist(), k
    assert a["est_index"].tolist() == [1, 0, 3, 2, 4] and a["group_tri"].tolist() == [0, 3, 3] and a["n_tri"] == 3
    assert a["tri_early"].tolist() == [1, 1, 0] and a["tri_late"].tolist() == [0, 3, 3]
    assert pe.plan_nms(est, images=[(2, 1)])["est_index"].tolist() == [4]
    # the chain a - b - c: b is dropped by a, and c, near b only, is KEPT; a distance exactly at the limit keeps
    chain = np.array([1.0, 9.0, 1.0], np.float32)
    assert po.nms(b, chain, np.array([5.0, 5.0, 5.0])).tolist() == [1, 0, 1, 1, 1]
    assert po.nms(b, np.array([5.0, 9.0, 9.0], np.float32), np.array([5.0, 5.0, 5.0])).tolist() == [1, 1, 1, 1, 1]
    assert po.nms(b, np.array([9.0, 9.0, 1.0], np.float32), np.array([5.0, 5.0, 5.0])).tolist() == [1, 1, 0, 1, 1]
