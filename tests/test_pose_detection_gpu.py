"""GPU: pp_pose_match and pp_pose_nms through picopose_amd/pose_detection_eval.py against tests/pose_detection_oracle.py.  The matcher and
the walk take the errors as inputs, and nothing is accumulated in floating point on the device, so every table is compared bit for
bit, without a tolerance: hand-made errors over every group size the kernels branch on (a lane's first and second ground truth, an
empty side), values exactly at a limit, ties, +inf, NaN, ignored ground truths and duplicated rows, also on a side stream; hand-made
triangles for the walk; and the closed loop on tiny models, where the restatement runs on the errors `match_poses` returns, the
accumulation is bit-equal and the summaries agree to 1e-12 (a reordered mean of ~2000 values in [0, 1] moves by less than n 2^-53)."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_detection_oracle as po  # noqa: E402
import pose_error_oracle as peo  # noqa: E402

from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import pipeline  # noqa: E402
from picopose_amd import pose_detection_eval as pe  # noqa: E402  (absent before the feature: every test here fails without it)

gpu = pytest.mark.gpu
G_SIZES, E_SIZES = (0, 1, 3, 64, 65, 130), (0, 1, 7, 100)
M, T = 2, 10


def _rows(scene, im, obj, scores):
    n = len(scores)
    return {"scene_id": np.full(n, scene, np.int64), "im_id": np.full(n, im, np.int64), "obj_id": np.full(n, obj, np.int64),
            "score": np.asarray(scores, np.float64)}


def _cat(parts, keys):
    return {k: np.concatenate([p[k] for p in parts]) for k in keys}


@functools.lru_cache(maxsize=None)
def _match_case():
    """One group per (G_g, E_g) of the two size lists, in one call; errors drawn from the integers 0 .. 11, +inf and NaN, limits the
    integers 1 .. 10 (metric 0) and their halves (metric 1): errors exactly at a limit and ties are everywhere.  -> (plan, errors,
    limits, the oracle's tables, the first estimate and ground truth of the hand-made group), computed once and never modified."""
    rng = np.random.default_rng(5)
    est, ann = [], []
    for im, (G, E) in enumerate((g, e) for g in G_SIZES for e in E_SIZES):
        if G == 0 and E == 0:
            continue                                                           # (no record: no group)
        est.append(_rows(1, im, 1 + im % 3, np.round(rng.uniform(0, 1, E), 1)))       # equal scores: the lower row first
        ann.append(dict(_rows(1, im, 1 + im % 3, np.zeros(G)), ignore=rng.uniform(size=G) < 0.3))
    est, ann = _cat(est, ("scene_id", "im_id", "obj_id", "score")), _cat(ann, ("scene_id", "im_id", "obj_id", "ignore"))
    hand = int(np.flatnonzero((ann["im_id"] == G_SIZES.index(3) * len(E_SIZES) + E_SIZES.index(7)))[0])
    ann["ignore"][hand:hand + 3] = [True, False, False]
    plan = pe.plan_groups(est, ann, max_per_image=None)
    values = np.array(list(range(12)) + [np.inf, np.nan], np.float32)
    errors = values[rng.integers(0, len(values), (M, plan["n_pairs"]))]
    limits = np.broadcast_to(np.stack([np.arange(1.0, 11.0), np.arange(1.0, 11.0) / 2])[None], (len(plan["group_pair"]), M, T)).copy()
    for g in range(len(plan["group_pair"])):
        (_, ne), (g0, ng), off = plan["group_est"][g], plan["group_gt"][g], plan["group_pair"][g]
        block = errors[:, off:off + ne * ng].reshape(M, ne, ng)
        if ne >= 7 and ng >= 3:
            block[:, 1], block[:, 3] = block[:, 0], block[:, 2]                # duplicated rows
        if g0 == hand and ng == 3 and ne == 7:
            # the ignored ground truth 0 is nearest and 1, 2 tie: 1 wins, the twin row takes 2, the third copy is left with the ignored one;
            # then: exactly at the limit 4 next to +inf and NaN; only the ignored one qualifies; nothing qualifies
            block[0] = [[0.5, 2, 2], [0.5, 2, 2], [0.5, 2, 2], [np.inf, np.nan, 4], [3, 11, 11], [11, 11, 11], [np.nan, np.inf, 11]]
        errors[:, off:off + ne * ng] = block.reshape(M, -1)
    return plan, errors, limits, po.match(plan, errors, limits), hand


def _assert_tables_equal(got, ref):
    for k in po.TABLES:
        a, b = got[k], ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (k, np.flatnonzero(a.ravel() != b.ravel())[:8])


@gpu
def test_match_tables_equal_the_scan_for_every_group_size_and_on_a_side_stream():
    plan, errors, limits, ref, hand = _match_case()
    assert set(G_SIZES) <= set(plan["group_gt"][:, 1].tolist()) and set(E_SIZES) <= set(plan["group_est"][:, 1].tolist())
    got = pe.match_pose_errors(plan, errors, limits)
    _assert_tables_equal(got, ref)
    assert (got["est_match"] >= 0).any() and (got["est_match"] < 0).any() and got["est_ignore"].any() and (got["gt_match"] >= 0).any()
    # the hand-made group, metric 0: at the limit 3 (t = 2) the ignored ground truth is nearest, yet the tie of the other two goes to
    # the lowest index, the twin row takes the next one and the third copy is left with the ignored one; at the limit 2 (t = 1) the
    # errors of 2 are exactly at the limit and only the ignored ground truth qualifies: matched, and ignored
    e0 = int(plan["group_est"][(plan["group_gt"][:, 0] == hand) & (plan["group_est"][:, 1] == 7)][0, 0])
    assert got["est_match"][0, 2, e0:e0 + 7].tolist() == [hand + 1, hand + 2, hand, -1, -1, -1, -1]
    assert got["est_ignore"][0, 2, e0:e0 + 7].tolist() == [0, 0, 1, 0, 0, 0, 0]
    assert got["est_match"][0, 1, e0:e0 + 5].tolist() == [hand, -1, -1, -1, -1] and got["est_ignore"][0, 1, e0] == 1
    assert got["gt_match"][0, 2, hand:hand + 3].tolist() == [e0 + 2, e0, e0 + 1]
    # a tensor on the device and a side stream give the same bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = pe.match_pose_errors(plan, torch.from_numpy(errors).cuda(), limits)
    side.synchronize()
    _assert_tables_equal(other, ref)
    # one metric, one threshold: M and T are free
    one = pe.match_pose_errors(plan, errors[1:], limits[:, 1:, 4:5])
    _assert_tables_equal(one, po.match(plan, errors[1:], limits[:, 1:, 4:5]))
    assert np.array_equal(one["est_match"][0, 0], ref["est_match"][1, 4])


@gpu
def test_match_exactly_at_the_limit_and_after_the_twin_was_taken():
    """Two estimates, three ground truths (the first ignored), written out: the restatement's answers are asserted by hand in
    test_pose_detection_cpu.py; the device gives the same tables."""
    est = _rows(1, 1, 5, [0.9, 0.8])
    ann = dict(_rows(1, 1, 5, np.zeros(3)), ignore=np.array([True, False, False]))
    plan = pe.plan_groups(est, ann)
    limits = np.array([4.0, np.nextafter(4.0, 5.0)]).reshape(1, 1, 2)
    for block, want, ign in (([[0.5, 2, 2], [np.inf, np.nan, 4]], [[1, -1], [1, 2]], [[0, 0], [0, 0]]),
                             ([[0.5, 9, 9], [-0.0, 9, 9]], [[0, -1], [0, -1]], [[1, 0], [1, 0]])):
        err = np.array(block, np.float32).ravel()[None]
        got = pe.match_pose_errors(plan, err, limits)
        _assert_tables_equal(got, po.match(plan, err, limits))
        assert got["est_match"][0].tolist() == want and got["est_ignore"][0].tolist() == ign


@gpu
def test_nms_walk_equals_the_restatement_on_hand_made_triangles():
    rng = np.random.default_rng(9)
    sizes = (1, 2, 64, 65, 130, 3)
    est = _cat([dict(_rows(2, im, 4, np.round(rng.uniform(0, 1, E), 1) if im % 2 else np.full(E, 0.5)), R=np.zeros((E, 3, 3)), t=np.zeros((E, 3)))
                for im, E in enumerate(sizes)], ("scene_id", "im_id", "obj_id", "score", "R", "t"))
    plan, ref_plan = pe.plan_nms(est), po.plan_nms(est)
    assert plan["group_est"][:, 1].tolist() == list(sizes) and plan["n_tri"] == sum(E * (E - 1) // 2 for E in sizes)
    for k in ("group_est", "group_tri", "est_index", "tri_early", "tri_late"):
        assert plan[k].tolist() == ref_plan[k].tolist(), k
    dist = rng.integers(0, 40, plan["n_tri"]).astype(np.float32)             # limit 4: a tenth of the pairs are near, some exactly at 4
    dist[rng.integers(0, len(dist), 50)] = np.nan
    off = int(plan["group_tri"][5])
    dist[off:off + 3] = [1, 9, 1]                                             # a - b - c: b is dropped by a; c, near b only, is KEPT
    off = int(plan["group_tri"][1])
    dist[off] = 4                                                             # exactly at the limit: kept
    limit = np.full(len(sizes), 4.0)
    keep = pe.nms_walk(plan, dist, limit)
    ref = po.nms(ref_plan, dist, limit)
    assert keep.dtype == ref.dtype and keep.tobytes() == ref.tobytes(), np.flatnonzero(keep != ref)[:8]
    e5, e1 = int(plan["group_est"][5, 0]), int(plan["group_est"][1, 0])
    assert keep[e5:e5 + 3].tolist() == [1, 0, 1] and keep[e1:e1 + 2].tolist() == [1, 1] and keep[0] == 1
    assert 0 < keep.sum() < len(keep) and all(keep[s:s + n].sum() < n for s, n in plan["group_est"][2:5])
    # a limit of 0 keeps everything, an infinite one keeps the first of each group (no NaN among its partners) or what the NaNs spare
    assert pe.nms_walk(plan, dist, np.zeros(len(sizes))).all()
    wide = pe.nms_walk(plan, np.nan_to_num(dist, nan=7.0), np.full(len(sizes), np.inf))
    assert wide.tolist() == po.nms(ref_plan, np.nan_to_num(dist, nan=7.0), np.full(len(sizes), np.inf)).tolist() and wide.sum() == len(sizes)
    with torch.cuda.stream(torch.cuda.Stream()):
        again = pe.nms_walk(plan, torch.from_numpy(dist).cuda(), limit)
    assert again.tobytes() == ref.tobytes()


def _closed_loop_set():
    """2 scenes x 3 images; objects 1 (a cube of 8 vertices, its 24 rotations) and 2 (the same vertices, a continuous symmetry about z).
    Per image two instances of object 1 (400 mm apart) and one of object 2; image (1, 0) holds a third instance of object 1 seen 5 %.
    Estimates per instance: the ground-truth pose (the top score of its image), an exact duplicate, a copy moved by 0.3 diameters, and
    per image one far-off pose.  The scores fall from image to image, so a duplicate in one image outranks the true poses of the next."""
    rng = np.random.default_rng(3)
    V = np.array([[x, y, z] for x in (-1.0, 1) for y in (-1.0, 1) for z in (-1.0, 1)], np.float32) * 40
    diam = 80.0 * math.sqrt(3.0)
    objects = {1: {"vertices": V, "info": {"diameter": diam, "symmetries_discrete": peo.cube_symmetries()}},
               2: {"vertices": V, "info": {"diameter": diam, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}}
    K = np.array([[600.0, 0, 320], [0, 600, 240], [0, 0, 1]])
    gt, info, cams, lines, kinds = {}, {}, {}, [], []
    base = 0.95
    for s in (1, 2):
        gt[s], info[s], cams[s] = {}, {}, {}
        for im in range(3):
            ids = [1, 1, 2] + ([1] if (s, im) == (1, 0) else [])
            R = np.array([peo.random_rotation(rng) for _ in ids])
            t = np.array([[-200.0 + 400 * k, 30.0 * k - 150 * (k == 3), 900 + 50.0 * k] for k in range(len(ids))])
            gt[s][im] = {"obj_id": np.array(ids, np.int64), "R": R, "t": t}
            info[s][im] = [{"visib_fract": 0.05 if k == 3 else 0.8} for k in range(len(ids))]
            cams[s][im] = {"K": K, "depth_scale": 1.0}
            rows = []
            for k, o in enumerate(ids):
                shift = 0.3 * diam * np.array([0.6, 0.0, 0.8])
                rows += [("true", o, base, R[k], t[k]), ("duplicate", o, base - 0.05, R[k], t[k]), ("moved", o, base - 0.07, R[k], t[k] + shift)]
            rows.append(("far", 1, 0.01, R[0], t[0] + [0.0, 1000.0, 0.0]))
            for kind, o, score, Rk, tk in rows:
                preds = [[{"R_stage_3": Rk.ravel(), "t_stage_3": tk}]]
                lines += pipeline.bop_csv_lines(s, im, [o], [score], preds, 0.25)
                kinds.append(kind)
            base -= 0.1
    return objects, gt, info, cams, lines, np.array(kinds)


@gpu
def test_closed_loop_scores_duplicates_down_and_nms_removes_exactly_them():
    objects, gt, info, cams, lines, kinds = _closed_loop_set()
    models = ev.ObjectModels(objects)
    assert [models.n_symmetries(o) for o in (1, 2)] == [24, 315]
    est = ev.read_bop_results(lines)
    ann = pe.pose_annotations(gt, info)
    assert ann["ignore"].sum() == 1 and len(est["score"]) == len(kinds) == 6 * 10 + 3
    got = pe.match_poses(est, ann, models, cams)
    ref_plan = po.plan(est, po.annotations(gt, info))
    for k in po.LAYOUT:
        assert got[k].dtype == ref_plan[k].dtype and got[k].tobytes() == ref_plan[k].tobytes(), k
    assert got["images"] == ref_plan["images"] and got["objects"] == ref_plan["objects"] == [1, 2]
    assert got["errors"].dtype == np.float32 and got["errors"].shape == (2, ref_plan["n_pairs"]) and got["limits"].shape == (12, 2, 10)
    assert got["limits"][0, 0].tolist() == (models.diameter(1) * ev.MSSD_THRESHOLDS).tolist() and got["limits"][0, 1].tolist() == ev.MSPD_THRESHOLDS.tolist()
    ref = po.match(ref_plan, got["errors"], got["limits"])
    _assert_tables_equal(got, ref)
    acc, acc_ref = pe.accumulate(got), po.accumulate(dict(ref_plan, metrics=got["metrics"], **ref))
    assert acc["precision"].tobytes() == acc_ref["precision"].tobytes() and acc["recall"].tobytes() == acc_ref["recall"].tobytes()
    before, s_ref = pe.summarize(acc), po.summarize(acc_ref)
    for k in ("AP", "AP_MSSD", "AP_MSPD"):
        assert abs(before[k] - s_ref[k]) <= 1e-12, k
    assert 0 < before["AP"] < 1 and np.all(acc["recall"] == 1)                  # every counted instance is found; the rest are false positives
    # every true pose matches its own instance at every threshold, the one on the 5 % instance is ignored
    true_rows = np.flatnonzero(kinds == "true")
    on_axis = np.isin(got["est_index"], true_rows)
    assert (got["est_match"][:, :, on_axis] >= 0).all() and got["est_ignore"][:, :, on_axis].sum() == 2 * 10
    # the suppression removes exactly the duplicates, from the dict and from the lines
    keep = pe.pose_nms(est, models)
    assert keep.tolist() == np.flatnonzero(kinds != "duplicate").tolist()
    kept_lines = pipeline.suppress_duplicate_poses(["scene_id,im_id,obj_id,score,R,t,time\n"] + lines, models)
    assert kept_lines == ["scene_id,im_id,obj_id,score,R,t,time\n"] + [lines[i] for i in keep]
    kept_rows = pipeline.suppress_duplicate_poses(est, models)
    assert all(np.array_equal(kept_rows[k], est[k][keep]) for k in est)
    after = pe.score_pose_detections(kept_rows, ann, models, cams)
    assert before["AP"] < after["AP"] < 1, (before["AP"], after["AP"])
    clean = pe.score_pose_detections({k: v[true_rows] for k, v in est.items()}, ann, models, cams)
    for k in ("AP", "AP_MSSD", "AP_MSPD"):
        assert abs(clean[k] - 1) <= 1e-12, (k, clean[k])
    assert abs(clean["per_object"][2]["AP"] - 1) <= 1e-12
    # the images filter and the per-image cut reach the device path too
    few = pe.match_poses(est, ann, models, cams, images=[(2, 1), (1, 0)], max_per_image=4)
    ref_few = po.plan(est, po.annotations(gt, info), images=[(2, 1), (1, 0)], max_per_image=4)
    assert few["images"] == [(1, 0), (2, 1)] and few["est_index"].tobytes() == ref_few["est_index"].tobytes() and len(few["est_index"]) == 8
    _assert_tables_equal(few, po.match(ref_few, few["errors"], few["limits"]))
