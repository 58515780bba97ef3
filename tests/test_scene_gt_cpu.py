"""CPU: the scene-ground-truth oracle (tests/scene_gt_oracle.py) against fixed answers that do not come from it (closed forms on the
plate, counts computed with tests/vsd_oracle.py alone), the float64 definition, the host side of picopose_amd/scene_gt.py — the
whole-image group planner, every ValueError, the file schema, targets, run lengths, detection records — and the argument checks of
pp_scene_gt / pp_scene_gt_workspace_bytes through the ABI (no GPU)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_gt_oracle as so  # noqa: E402
import scene_tables as st  # noqa: E402
import vsd_oracle as vo  # noqa: E402

from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import scene_gt as sg  # noqa: E402  (absent before the feature: every test here fails without it)
from picopose_amd.provider import test_batch as tb  # noqa: E402

F = np.float32
PH, PW = vo.PLATE_HW


def _mixed_views():
    ms = vo.mixed_scene()
    return {"objects": ms["objects"], "obj_ids": ms["obj_ids"], "image_index": ms["image_index"], "R": ms["R_gt"], "t": ms["t_gt"], "cams": vo.CAMS,
            "depth": vo.depth_mm32(ms["depth_u16"], ms["depth_scale"])}


@functools.lru_cache(maxsize=None)
def _edge_ref():
    return so.scene_reference(so.edge_scene(), vo.H, vo.W)


@functools.lru_cache(maxsize=None)
def _mixed_ref(pad="bop"):
    return so.scene_reference(_mixed_views(), vo.H, vo.W, pad)


PLATE_ROWS = [((0, 0, 500), 256, (33, 23, 48, 38), (33, 23, 48, 38), 1.0), ((-200, 0, 500), 144, (-7, 23, 8, 38), (0, 23, 8, 38), 0.5625),
              ((-200, -150, 500), 81, (-7, -7, 8, 8), (0, 0, 8, 8), 81 / 256), ((235, 180, 500), 6, (80, 59, 95, 74), (80, 59, 82, 60), 6 / 256),
              ((-400, 0, 500), 0, (-47, 23, -32, 38), so.EMPTY, 0.0)]


def _plate_rows_scene():
    n = len(PLATE_ROWS)
    return dict(so.plate_scene([r[0] for r in PLATE_ROWS]), image_index=np.arange(n, dtype=np.int32), cams=np.array([vo.PLATE_K4] * n, dtype=F),
                depth=np.zeros((n, PH, PW), dtype=F))


def test_plate_rows_on_the_bop_canvas_and_on_the_frame():
    """The 16 x 16-sample plate moved over the borders of the 61 x 83 frame, the depth all missing: on the canvas of pad (83, 61) every row
    keeps its 256 samples and its whole box, the visible count is the in-frame count, and the plate 400 mm to the left is off the frame
    (empty visible box) but on the canvas.  With pad (0, 0) `all` and bbox_obj shrink to the in-frame values."""
    scene = _plate_rows_scene()
    r = so.scene_reference(scene, PH, PW, (83, 61))
    r0 = so.scene_reference(scene, PH, PW, (0, 0))
    for k, (_, inframe, bo, bv, fract) in enumerate(PLATE_ROWS):
        assert tuple(r["counts"][k]) == (256, 0, inframe) and r["inframe"][k] == inframe, (k, r["counts"][k])
        assert tuple(r["bbox_obj"][k]) == bo and tuple(r["bbox_visib"][k]) == bv, (k, r["bbox_obj"][k], r["bbox_visib"][k])
        assert r["counts"][k, 2] / r["counts"][k, 0] == fract
        assert tuple(r0["counts"][k]) == (inframe, 0, inframe) and tuple(r0["bbox_obj"][k]) == bv == tuple(r0["bbox_visib"][k])
        assert r["mask_visib"][k].sum() == 255 * inframe and np.array_equal(r["mask_all"][k], r["mask_visib"][k])
    # the occluder depth of the VSD plate cases: 300 mm over the plate's left eight columns, MISSING everywhere else.  The left half is
    # hidden, the right half is visible because its depth is missing: visib 128.  px_count_valid counts Z_test > 0, so it is the 128
    # samples under the occluder (the feature request's prose quoted 256 for it, which contradicts its own definition of the count and
    # its edge-scene table, where valid = in-frame - missing; the definition is what is asserted here).
    occ = vo.plate_cases()["occluder"][2]
    assert (occ > 0).sum() == 8 * PH
    one = so.scene_reference(so.plate_scene([(0, 0, 500)]), PH, PW, (83, 61), occ[None])
    assert tuple(one["counts"][0]) == (256, 128, 128) and tuple(one["bbox_visib"][0]) == (41, 23, 48, 38)
    assert tuple(one["bbox_obj"][0]) == (33, 23, 48, 38)


def test_composite_closed_forms_of_two_plates():
    """No depth: a plate at 400 mm (20 x 20 samples) in front of one at 500 mm shifted by 12 columns hides 6 x 16 of its 256 samples at
    delta 0 and 15 (D differs by about 100 mm) and none at delta 150; two identical views tie, and the lower label wins everywhere."""
    two = so.plate_scene([(0, 0, 400), (60, 0, 500)])
    for delta, visib in ((0.0, 160), (15.0, 160), (150.0, 256)):
        r = so.scene_reference(two, PH, PW, "bop", None, delta)
        assert r["counts"].tolist() == [[400, 400, 400], [256, 256, visib]], (delta, r["counts"])
        assert r["bbox_obj"].tolist() == [[31, 21, 50, 40], [45, 23, 60, 38]]
    assert (r["instance_map"][0] == 0).sum() == 400 and (r["instance_map"][0] == 1).sum() == 160 and (r["instance_map"][0] == -1).sum() == PH * PW - 560
    assert np.array_equal(r["scene_depth"][0] > 0, r["instance_map"][0] >= 0)
    same = so.scene_reference(so.plate_scene([(0, 0, 500), (0, 0, 500)]), PH, PW, "bop", None, 0.0)
    assert set(np.unique(same["instance_map"])) == {-1, 0} and same["counts"].tolist() == [[256, 256, 256]] * 2
    z = np.full((2, 3), 7.0, dtype=F)
    assert np.all(so.composite([z, z], labels=[5, 2])[1] == 5) and np.all(so.composite([z, z - 1], labels=[5, 2])[1] == 2)


def test_edge_scene_counts():
    want = [(468, 319, 319, 123, 0), (467, 265, 265, 265, 0), (409, 238, 238, 238, 0), (394, 101, 101, 101, 0), (97200, 10800, 10650, 10800, 184),
            (256, 32, 32, 0, 0), (0, 0, 0, 0, 12), (293, 293, 146, 293, 0), (271, 271, 137, 184, 0)]
    r = _edge_ref()
    got = np.c_[r["counts"][:, 0], r["inframe"], r["counts"][:, 1:], r["near"]]
    assert got.tolist() == [list(w) for w in want], got
    assert tuple(r["bbox_obj"][4]) == (-120, -90, 239, 179) and tuple(r["bbox_visib"][4]) == (0, 0, 119, 89)      # the whole canvas / frame
    assert tuple(r["bbox_visib"][5]) == so.EMPTY and tuple(r["bbox_obj"][6]) == so.EMPTY and r["bbox_obj"][5][0] < 0 <= r["bbox_obj"][5][2]


def test_mixed_scene_counts_with_depth_and_composite():
    all_ = [317, 920, 305, 623, 240, 303, 215, 334, 149, 335, 281, 229]
    visib = [183, 920, 157, 282, 240, 238, 92, 15, 44, 319, 128, 83]
    for pad in ((0, 0), "bop"):
        r = _mixed_ref(pad)
        assert r["counts"][:, 0].tolist() == all_ == r["counts"][:, 1].tolist() and r["counts"][:, 2].tolist() == visib, pad
    views = _mixed_views()
    c0 = so.scene_reference(views, vo.H, vo.W, "bop", None, 0.0)["counts"][:, 2].tolist()
    assert c0 == [183, 920, 305, 598, 240, 238, 159, 176, 44, 310, 281, 92]
    c15 = so.scene_reference(views, vo.H, vo.W, "bop", None, 15.0)["counts"][:, 2].tolist()
    assert [(k, v) for k, v in enumerate(c15) if v != c0[k]] == [(0, 185), (3, 609), (9, 320)]


def test_padding_changes_the_float32_projection_of_one_mixed_view():
    """Why a padded render is not the frame render's bits in general: cx + W changes the float32 projection.  One of the twelve views."""
    views = _mixed_views()
    differ = 0
    for z0, z1 in zip(_mixed_ref((0, 0))["z"], _mixed_ref("bop")["z"]):
        differ += not np.array_equal(z0.view(np.int32), z1[vo.H:2 * vo.H, vo.W:2 * vo.W].view(np.int32))
    assert differ == 1 and len(views["obj_ids"]) == 12


def test_float32_counts_equal_the_float64_definition():
    """Condition of the test, asserted on the oracle alone: none of the 21 views has a pixel whose float64 margin float32 cannot decide.
    Then the float32 counts must equal the float64 definition's exactly."""
    for r in (_edge_ref(), _mixed_ref()):
        assert np.all(r["fragile"] == 0), r["fragile"]
        assert np.array_equal(r["counts"], r["counts64"])
    assert len(_edge_ref()["fragile"]) + len(_mixed_ref()["fragile"]) == 21


# ---- host side ------------------------------------------------------------------------------------------------------------------------
def test_image_groups_hold_whole_images():
    cost = np.array([1000, 1000, 3000, 500, 500, 500], dtype=np.int64)
    img = np.array([0, 0, 1, 3, 3, 3], dtype=np.int32)
    fb = 800
    assert sg.image_groups(cost, img, fb, 1 << 30) == [(0, 6, 0, 4)]
    # budget = bound - 768; image 0: 2800, image 1: 3800, image 3: 2300; the empty image 2 costs its words inside a range
    assert sg.image_groups(cost, img, fb, 768 + 3800) == [(0, 2, 0, 1), (2, 3, 1, 2), (3, 6, 3, 4)]
    assert sg.image_groups(cost, img, fb, 768 + 6600) == [(0, 3, 0, 2), (3, 6, 3, 4)]            # 0..1: 6600; 0..3 would be 10500
    assert sg.image_groups(cost, img, fb, 768 + 6900) == [(0, 3, 0, 2), (3, 6, 3, 4)]
    assert sg.image_groups(cost[2:], img[2:], fb, 768 + 6900) == [(0, 4, 1, 4)]                  # 1..3: 3000 + 1500 + 3 * 800 = 6900
    with pytest.raises(ValueError, match="image 1"):
        sg.image_groups(cost, img, fb, 768 + 3799)
    assert sg.image_groups(cost[:0], img[:0], fb, 1000) == []


def _cpu_models(faces=True):
    objs = vo.objects()
    if not faces:
        del objs[2]["faces"]
    return ev.ObjectModels(objs, device="cpu")


def test_every_value_error_of_scene_gt_info():
    m = _cpu_models()
    R, t = np.tile(np.eye(3, dtype=F), (2, 1, 1)), np.tile(F([0, 0, 500]), (2, 1))
    K = np.array([[100.0, 0, 60], [0, 100.0, 45], [0, 0, 1]])
    d = np.zeros((2, vo.H, vo.W), dtype=np.uint16)
    ok = dict(models=m, obj_ids=[1, 2], R=R, t=t, K=K, depth=d, depth_scale=1.0)
    bad = [{"obj_ids": [1, 4]}, {"obj_ids": [1.0, 2.0]}, {"models": _cpu_models(faces=False)}, {"models": None}, {"R": R[:1]},
           {"t": t.astype(np.int64)}, {"K": K[:2]}, {"K": np.zeros((3, 3, 3))}, {"K": np.zeros((3, 3))}, {"depth": d[0]},
           {"depth": d.astype(np.int32)}, {"depth_scale": None}, {"depth_scale": -1.0}, {"depth": d.astype(F)}, {"depth": [[0]]},
           {"image_index": [0, 2]}, {"image_index": [0]}, {"image_index": [0.0, 1.0]}, {"delta": -1.0}, {"delta": float("nan")},
           {"delta": float("inf")}, {"delta": "15"}, {"near": -1.0}, {"near": 0.0}, {"window": "tight"}, {"workspace_bytes": 0},
           {"pad": "toolkit"}, {"pad": (-1, 0)}, {"pad": (1.5, 0)}, {"pad": 3}, {"pad": (1, 2, 3)}, {"pad": (30000, 30000)},
           {"masks": "visible"}, {"masks": True}, {"composite": 1}, {"composite": "yes"}, {"resolution": (vo.H, vo.W + 1)},
           {"resolution": (0, 5)}, {"resolution": 7}, {"depth": None, "depth_scale": None}, {"depth": None, "resolution": (vo.H, vo.W)},
           {"depth": None, "depth_scale": None, "resolution": (vo.H, vo.W), "image_index": [0, 1]},      # K is (3, 3): one image
           {"depth": None, "depth_scale": None, "resolution": (vo.H, vo.W), "workspace_bytes": 50000}]   # one image's views exceed the bound
    for kw in bad:
        with pytest.raises(ValueError):
            sg.scene_gt_info(**dict(ok, **kw))
        print("ValueError:", {k: v for k, v in kw.items() if k != "models"})
    empty = sg.scene_gt_info(m, np.zeros(0, dtype=np.int64), R[:0], t[:0], K, depth=d, depth_scale=1.0, masks="both", composite=True)
    assert tuple(empty["px_count_all"].shape) == (0,) and tuple(empty["bbox_visib"].shape) == (0, 4) and empty["visib_fract"].shape == (0,)
    assert tuple(empty["mask_all"].shape) == tuple(empty["mask_visib"].shape) == (0, vo.H, vo.W) and empty["n_groups"] == 0 == empty["near_count"]
    assert tuple(empty["scene_depth"].shape) == (2, vo.H, vo.W) and int(empty["instance_map"].max()) == -1 and float(empty["scene_depth"].max()) == 0
    assert sg._pad("bop", 48, 64) == (64, 48) and sg._pad((3, 0), 48, 64) == (3, 0)
    c = sg.canvas_cams(np.array([[100, 100, 63.25, 41.75]], dtype=F), 120, 90)
    assert c.dtype == F and c[0].tolist() == [100.0, 100.0, float(F(63.25) + F(120)), float(F(41.75) + F(90))]


def _result():
    return {"px_count_all": np.array([256, 256, 0, 10]), "px_count_valid": np.array([200, 0, 0, 10]), "px_count_visib": np.array([128, 0, 0, 1]),
            "bbox_obj": np.array([[33, 23, 48, 38], [-47, 23, -32, 38], [0, 0, -1, -1], [5, 6, 5, 6]]),
            "bbox_visib": np.array([[41, 23, 48, 38], [0, 0, -1, -1], [0, 0, -1, -1], [5, 6, 5, 6]]), "visib_fract": np.array([0.5, 0.0, 0.0, 0.1])}


def test_format_gt_info_boxes_and_the_empty_box():
    info = sg.format_gt_info(_result())
    assert info[0] == {"bbox_obj": [33, 23, 15, 15], "bbox_visib": [41, 23, 7, 15], "px_count_all": 256, "px_count_valid": 200, "px_count_visib": 128,
                       "visib_fract": 0.5}
    assert info[1]["bbox_obj"] == [-47, 23, 15, 15] and info[1]["bbox_visib"] == [-1, -1, -1, -1]
    assert info[2]["bbox_obj"] == [-1, -1, -1, -1] == info[2]["bbox_visib"] and info[3]["bbox_visib"] == [5, 6, 0, 0]
    assert all(type(v) is int for e in info for k, v in e.items() if k.startswith("px")) and type(info[0]["visib_fract"]) is float
    import json
    json.dumps(info)


def test_targets_from_gt_info_threshold_zero_rows_and_order():
    gt = {2: {5: {"obj_id": np.array([7, 3, 7, 7])}, 1: {"obj_id": np.array([3])}}, 1: {9: {"obj_id": np.array([4, 4])}}}
    fr = lambda *v: [{"visib_fract": x} for x in v]  # noqa: E731
    info = {2: {5: fr(0.1, 0.05, 0.5, 0.0999), 1: fr(1.0)}, 1: {9: fr(0.0, 0.09)}}
    rows = sg.targets_from_gt_info(gt, info)
    assert rows.dtype == np.int64 and rows.tolist() == [[2, 1, 3, 1], [2, 5, 7, 2]]            # 0.1 counts, 0.0999 does not; zero-count rows are dropped
    assert sg.targets_from_gt_info(gt, info, min_visib_fract=0.0).tolist() == [[1, 9, 4, 2], [2, 1, 3, 1], [2, 5, 3, 1], [2, 5, 7, 3]]
    assert sg.targets_from_gt_info(gt, info, min_visib_fract=2.0).shape == (0, 4)
    with pytest.raises(ValueError):
        sg.targets_from_gt_info(gt, {2: {5: fr(0.1), 1: fr(1.0)}, 1: {9: fr(0.0, 0.09)}})


def test_rle_from_mask_round_trips_through_the_detection_decoder():
    rng = np.random.default_rng(0)
    m = np.zeros((13, 9), dtype=np.uint8)
    m[3:8, 2:6] = 255
    m[10, 7] = 255
    for mask in (m, (rng.uniform(size=(13, 9)) < 0.4), np.ones((4, 5), dtype=bool)):
        rle = sg.rle_from_mask(mask)
        h, w = mask.shape
        assert rle["size"] == [h, w] and all(type(c) is int for c in rle["counts"])
        counts = tb.rle_counts(rle)
        back = np.repeat(np.arange(len(counts)) % 2, counts).reshape(w, h).T.astype(bool)
        assert np.array_equal(back, mask != 0)
        area, extent = tb.rle_area_extent(counts, h)
        ys, xs = np.where(mask != 0)
        assert area == len(xs) and extent == (ys.min(), ys.max(), xs.min(), xs.max())
    assert sg.rle_from_mask(np.zeros((6, 7)))["counts"] == [42] and tb.rle_area_extent(tb.rle_counts(sg.rle_from_mask(np.zeros((6, 7)))), 6) == (0, None)
    first = np.zeros((6, 7), dtype=np.uint8)
    first[0, 0] = first[1, 0] = 255
    assert sg.rle_from_mask(first)["counts"] == [0, 2, 40] and sg.rle_from_mask(np.ones((4, 5), dtype=bool))["counts"] == [0, 20]
    with pytest.raises(ValueError):
        sg.rle_from_mask(np.zeros(5))


def test_gt_detections_records():
    masks = np.zeros((3, 6, 7), dtype=np.uint8)
    masks[0, 2:4, 1:6] = 255
    masks[2, 5, 6] = 255
    res = {"mask_visib": masks, "bbox_visib": np.array([[1, 2, 5, 3], [0, 0, -1, -1], [6, 5, 6, 5]]), "px_count_visib": np.array([10, 0, 1])}
    dets = sg.gt_detections([4, 9, 4], res, scene_id=3, im_id=17, score=0.5, time=0.25)
    assert len(dets) == 2 and set(dets[0]) == {"scene_id", "image_id", "category_id", "bbox", "score", "time", "segmentation"}
    assert dets[0]["bbox"] == [1, 2, 5, 2] and dets[1]["bbox"] == [6, 5, 1, 1] and [d["category_id"] for d in dets] == [4, 4]
    assert (dets[0]["scene_id"], dets[0]["image_id"], dets[0]["score"], dets[0]["time"]) == (3, 17, 0.5, 0.25)
    assert tb.rle_area_extent(tb.rle_counts(dets[0]["segmentation"]), 6) == (10, (2, 3, 1, 5))
    assert tb.select_detections(dets) == ([0, 1], 0.25)
    with pytest.raises(ValueError):
        sg.gt_detections([4, 9, 4], {"bbox_visib": res["bbox_visib"]}, 3, 17)
    with pytest.raises(ValueError):
        sg.gt_detections([4, 9], res, 3, 17)


def test_scene_gt_abi_argument_validation_needs_no_gpu():
    from picopose_amd import _lib

    L = _lib.lib()
    assert {"pp_scene_gt", "pp_scene_gt_workspace_bytes"} <= set(_lib.declared_symbols())
    need = ctypes.c_size_t()
    assert L.pp_scene_gt_workspace_bytes(1000, 24, 0, ctypes.byref(need)) == 0 and need.value == 256 + 8192 + 24 * 8
    assert L.pp_scene_gt_workspace_bytes(1000, 24, 100, ctypes.byref(need)) == 0 and need.value == 256 + 8192 + 256 + 800
    assert L.pp_scene_gt_workspace_bytes(0, 32, 100, ctypes.byref(need)) == 0 and need.value == 256 + 256 + 800
    for args in ((-1, 24, 0), (10, 0, 0), (10, 2 ** 32, 0), (2 ** 62, 1, 0), (10, 10, -1), (10, 10, 2 ** 62)):
        assert L.pp_scene_gt_workspace_bytes(*args, ctypes.byref(need)) == -1, args
    assert L.pp_scene_gt_workspace_bytes(10, 10, 10, None) == -1
    buf, p = st.aligned_buffer()
    i32, f32, i64 = st.i32, st.f32, st.i64
    H, W = 28, 44                                                  # pad (10, 10): the canvas is 48 x 64
    front = 256 + 1792 + 5 * 8                                     # 200 window samples, 2 + 2 + 1 faces
    # the FRAME cameras and frame size in the scene; the windows lie on the canvas; the device table `diameters` is not read: null
    scene = dict(st.fields(p, H, W), cams_host=f32(100, 100, 22, 14, 90, 95, 20.5, 10), diameters=None)
    own = dict(canvas_cams=p, canvas_cams_host=f32(100, 100, 32, 24, 90, 95, 30.5, 20), pad_x=10, pad_y=10, depth=p, delta=15.0, view_label=p,
               use_view_label=1, workspace=p, workspace_bytes=front, counts=p, boxes=p, near_count=p, mask_all=None, mask_visib=None,
               scene_depth=None, instance_map=None)
    call = st.caller(L.pp_scene_gt, scene, own)

    comp = 2304 + 2 * H * W * 8                                    # the front rounded up to 256, then the words of two images
    assert call(scene=None) == -1
    for k in [k for k in st.DEVICE_TABLES if k != "diameters"] + [k for k in own if own[k] is p and k != "depth"] + list(st.HOST_TABLES) + ["canvas_cams_host"]:
        assert call(**{k: None}) == -1, k
    for kw in ({"n_objects": 0}, {"n_images": 0}, {"n_views": 0}, {"H": 0}, {"W": -3},
               {"pad_x": -1, "canvas_cams_host": f32(100, 100, 21, 24, 90, 95, 19.5, 20)}, {"pad_y": -1},
               {"H": 50000, "W": 50000, "pad_x": 0, "pad_y": 0, "canvas_cams_host": f32(100, 100, 22, 14, 90, 95, 20.5, 10)},
               {"pad_x": 2 ** 30}, {"pad_y": 25000, "pad_x": 25000},
               {"delta": -1.0}, {"delta": float("inf")}, {"delta": float("nan")}, {"near": 0.0}, {"near": float("inf")}, {"near": float("nan")},
               {"canvas_cams_host": f32(100, 100, 32, 24, 90, 95, 30.5, 20.5)}, {"canvas_cams_host": f32(100, 100, 32, 24, 91, 95, 30.5, 20)},
               {"canvas_cams_host": f32(100, 100, 22, 14, 90, 95, 20.5, 10)}, {"cams_host": f32(100, 100, 22, 14, 90, float("nan"), 20.5, 10)},
               {"cams_host": f32(0, 100, 22, 14, 90, 95, 20.5, 10), "canvas_cams_host": f32(0, 100, 32, 24, 90, 95, 30.5, 20)},
               {"diameters_host": f32(100.0, 0.0)}, {"vert_off_host": i32(1, 4, 7)}, {"vert_off_host": i32(0, 4, 4)}, {"face_off_host": i32(0, 2, 1)},
               {"face_off_host": i32(0, 3, 3)}, {"faces_host": i32(0, 1, 2, 0, 2, 4, 0, 1, 2)}, {"faces_host": i32(0, -1, 2, 0, 2, 3, 0, 1, 2)},
               {"view_obj_host": i32(0, 2, 1)}, {"view_img_host": i32(0, -1, 1)}, {"windows_host": i32(0, 0, 10, 10, 55, 38, 65, 48, 5, 5, 5, 9)},
               {"windows_host": i32(0, 0, 10, 10, 54, 39, 64, 49, 5, 5, 5, 9)}, {"windows_host": i32(-1, 0, 9, 10, 54, 38, 64, 48, 5, 5, 5, 9)},
               {"windows_host": i32(0, 0, 10, 10, 54, 38, 64, 48, 6, 5, 5, 9)}, {"view_zoff_host": i64(0, 100, 200, 201)},
               {"view_zoff_host": i64(1, 101, 201, 201)}):
        assert call(**kw) == -1, kw
    # PP_EWORKSPACE: the front alone with a depth image; the composite's words when it runs (no depth, or an output asked for).  These
    # calls pass every check of the scene first (with `diameters` null), so they also guard the ctypes layout of _lib.PpScene.
    assert call(workspace_bytes=front - 1) == -2 and call(workspace=p + 64) == -2 and call(workspace_bytes=0) == -2
    assert call(depth=None) == -2 and call(depth=None, workspace_bytes=comp - 1) == -2
    assert call(scene_depth=p, workspace_bytes=comp - 1) == -2 and call(instance_map=p, workspace_bytes=comp - 1) == -2
    assert call(mask_all=p, mask_visib=p, workspace_bytes=front - 1) == -2
