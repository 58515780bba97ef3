"""GPU: pp_det_overlaps and pp_det_match through picopose_amd/detection_eval.py against tests/detection_eval_oracle.py: every table
(inter, iou as float64 bits, dt_match, dt_ignore, gt_match, gt_ignore) bit for bit — nothing is accumulated in floating point on the
device, so there is no tolerance — for both IoU types, two frame sizes in one call, every group size the kernels branch on, IoUs exactly
at a threshold, crowds, ignored and duplicated ground truths, empty masks, area-range edges; the same bits under a chunking that splits the
images and on a side stream; accumulate exactly, the summaries to 1e-12 (a reordered mean of at most ~1e5 values in [0, 1] moves by
less than n 2^-53); and the closed loop from a rendered scene's ground truth to the twelve numbers."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detection_eval_oracle as eo  # noqa: E402
import vsd_oracle as vo  # noqa: E402

from picopose_amd import detection_eval as de  # noqa: E402  (absent before the feature: every test here fails without it)
from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import scene_gt as sg  # noqa: E402

gpu = pytest.mark.gpu
KW = {"segm": {"area_ranges": eo.SMALL_RANGES}, "bbox": {"iou_type": "bbox", "area_ranges": eo.SMALL_RANGES}}


@functools.lru_cache(maxsize=None)
def _reference(iou_type):
    """The oracle's tables of the random case, computed once per IoU type and never modified."""
    dets, anns = eo.random_case(0)
    return eo.match(list(dets), list(anns), **KW[iou_type])


def _assert_tables_equal(got, ref):
    for k in eo.TABLES + eo.LAYOUT:
        a, b = got[k], ref[k]
        if b is None:
            assert a is None, k
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (k, np.flatnonzero(a.ravel() != b.ravel())[:8])
    assert got["images"] == ref["images"] and got["categories"] == ref["categories"]


@gpu
@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_tables_equal_the_oracle_chunked_and_on_a_side_stream(iou_type):
    dets, anns = (list(v) for v in eo.random_case(0))
    ref = _reference(iou_type)
    got = de.match_detections(dets, anns, **KW[iou_type])
    _assert_tables_equal(got, ref)
    assert got["n_chunks"] == (2 if iou_type == "segm" else 1)                       # two frame sizes: two pack calls
    assert {0, 1, 3, 64, 65, 130} <= set(got["group_gt"][:, 1].tolist()) and {0, 1, 7, 100} <= set(got["group_det"][:, 1].tolist())
    assert (got["dt_match"] >= 0).any() and got["dt_ignore"].any() and (got["iou"] == 1).any() and (got["iou"] == 0).any()
    split = de.match_detections(dets, anns, workspace_bytes=20000, **KW[iou_type])
    assert split["n_chunks"] >= 4
    _assert_tables_equal(split, ref)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = de.match_detections(dets, anns, **KW[iou_type])
    side.synchronize()
    _assert_tables_equal(other, ref)
    # accumulation: the same float64 operations in the same order on the same integers
    acc, acc_ref = de.accumulate(got), eo.accumulate(ref)
    assert acc["precision"].tobytes() == acc_ref["precision"].tobytes() and acc["recall"].tobytes() == acc_ref["recall"].tobytes()
    s, s_ref = de.summarize(acc), eo.summarize(acc_ref)
    for k in eo.NAMES:
        assert abs(s[k] - s_ref[k]) <= 1e-12, k
    assert 0 < s["AP"] < 1 and s["per_object_AP"].keys() == s_ref["per_object_AP"].keys()


@gpu
def test_thresholds_crowds_and_twins_on_the_device():
    dets, anns = (list(v) for v in eo.threshold_case())
    got = de.match_detections(dets, anns)
    _assert_tables_equal(got, eo.match(dets, anns))
    iou = got["iou"].reshape(5, 5)
    assert got["inter"].reshape(5, 5)[0, 0] == 8 and iou[0, 0] == 0.5 and iou[1, 1] == 0.75 and iou[2, 2] == 1.0 == iou[3, 2]
    assert got["dt_match"][0, :, 0].tolist() == [0] + [-1] * 9 and got["dt_match"][0, :, 1].tolist() == [1] * 6 + [-1] * 4
    assert got["dt_match"][0, 0].tolist() == [0, 1, 2, 2, 4] and got["gt_match"][0, 0].tolist() == [0, 1, 3, -1, 4]
    # class-agnostic scoring and a custom threshold list, against the oracle
    kw = {"class_agnostic": True, "iou_thrs": [0.25, 0.5, 1.0], "max_dets": (2, 3)}
    mixed = [dict(d, category_id=1 + i % 2) for i, d in enumerate(dets)]
    _assert_tables_equal(de.match_detections(mixed, anns, **kw), eo.match(mixed, anns, **kw))
    s, s_ref = de.score_detections(mixed, anns, **kw), eo.score(mixed, anns, **kw)
    assert all(abs(s[k] - s_ref[k]) <= 1e-12 for k in eo.NAMES) and s["AR100"] == -1 and s["AP75"] == -1      # positions the settings lack


@gpu
def test_segm_overlaps_over_a_second_part_filled_staging_step():
    """A 48 x 64 frame is 96 words: the segm overlaps kernel stages 64 words per step, so it runs a second step, part-filled (the
    frames of the random case are 15 and 34 words: one step).  9 detections against 3 ground truths and 1 against 9: both sides
    cross a tile edge of 8.  Counts are integers and an IoU is one division: no tolerance."""
    dets, anns = eo.image_case(np.random.default_rng(4), 48, 64, 1, 1, {1: (9, 3), 2: (1, 9)})
    ref = eo.match(dets, anns)
    # the case is worth its name: a share of the intersecting pixels lies in the words 64 .. 95, the pixels 2048 and up of the run order
    late = [eo.do.decode(r["segmentation"]).ravel(order="F")[2048:] > 0 for r in dets + anns]
    pairs = [(i, len(dets) + j) for i, d in enumerate(dets) for j, a in enumerate(anns) if d["category_id"] == a["category_id"]]
    second = sum(int((late[i] & late[j]).sum()) for i, j in pairs)
    assert (ref["inter"] > 0).sum() >= 20 and 0 < second < ref["inter"].sum() < 2 * second
    got = de.match_detections(dets, anns)
    assert got["n_chunks"] == 1 and got["inter"].shape == (9 * 3 + 1 * 9,)
    _assert_tables_equal(got, ref)


@gpu
def test_closed_loop_from_scene_ground_truth_to_the_twelve_numbers():
    """Two instances of the 16-sample plate (one mesh under two object ids: with one category per instance AR1 is 1 as well) in a
    40 x 48 frame, composite visibility: the ground truth's own masks as detections score 1;
    with one detection's score lowered and its mask replaced by a disjoint one the result equals the oracle and AP drops."""
    H, W = 40, 48
    p = vo.plate(vo.PLATE_N)
    models = ev.ObjectModels({o: {"vertices": p["vertices"], "faces": p["faces"], "info": {"diameter": vo.PLATE_DIAMETER}} for o in (3, 4)})
    K = vo.k33(np.array([(100.0, 100.0, 23.5, 19.5)], dtype=np.float32))[0].astype(np.float64)
    ids, R, t = np.array([3, 4]), np.stack([np.eye(3)] * 2), np.array([[-50.0, 0, 500], [55.0, 10, 500]])
    r = sg.scene_gt_info(models, ids, R, t, K, depth=None, resolution=(H, W), masks="visib")
    assert r["px_count_visib"].tolist() == [256, 256]
    anns = de.gt_annotations(ids, r, scene_id=2, im_id=5)
    dets = sg.gt_detections(ids, r, scene_id=2, im_id=5)
    assert len(anns) == 2 and not any(a["ignore"] or a["iscrowd"] for a in anns) and [a["bbox"] for a in anns] == [d["bbox"] for d in dets]
    whole = de.dataset_annotations({2: {5: {"obj_id": ids, "R": R, "t": t}}}, {2: {5: {"K": K, "depth_scale": 1.0}}}, models, (H, W))
    assert whole == anns
    for iou_type in ("segm", "bbox"):
        s = de.score_detections(dets, anns, iou_type=iou_type)
        defined = [k for k in eo.NAMES if s[k] != -1]
        assert {"AP", "AP50", "AP75", "APs", "AR1", "AR10", "AR100", "ARs"} <= set(defined) and s["APl"] == -1
        for k in defined:
            assert abs(s[k] - 1) <= 1e-12, (iou_type, k, s[k])
        assert abs(s["per_object_AP"][3] - 1) <= 1e-12 and abs(s["per_object_AP"][4] - 1) <= 1e-12
        away = eo.rect(H, W, 30, 38, 20, 26)
        worse = [dets[0], dict(eo.det(away, 0.5, cat=4, scene=2, image=5), time=0.0)]
        s2, s2_ref = de.score_detections(worse, anns, iou_type=iou_type), eo.score(worse, anns, iou_type=iou_type)
        assert all(abs(s2[k] - s2_ref[k]) <= 1e-12 for k in eo.NAMES) and 0 < s2["AP"] < 1 - 1e-3, (iou_type, s2)
        _assert_tables_equal(de.match_detections(worse, anns, iou_type=iou_type), eo.match(worse, anns, iou_type=iou_type))
