"""GPU: pp_scene_gt (picopose_amd/scene_gt.py) against tests/scene_gt_oracle.py: counts, boxes and masks equal to the numpy restatement
for both canvases and both windows and under a workspace bound that forces several calls; tied to the existing kernels (vsd_errors'
visible count, render_depth's coverage); the edge scene, the plate rows and a NaN pose; composite visibility, scene_depth and
instance_map with the tie rule; determinism across view order, stream and grouping; U = 0; and the three uses end to end."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detections_oracle as do  # noqa: E402
import render_oracle as ro  # noqa: E402
import scene_gt_oracle as so  # noqa: E402
import vsd_oracle as vo  # noqa: E402

from picopose_amd import _lib  # noqa: E402
from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import scene as scn  # noqa: E402
from picopose_amd import scene_gt as sg  # noqa: E402  (absent before the feature: every test here fails without it)
from picopose_amd.provider import test_batch as tb  # noqa: E402
from picopose_amd.utils.preprocess import get_bbox  # noqa: E402

gpu = pytest.mark.gpu
F = np.float32
KEYS = ("px_count_all", "px_count_valid", "px_count_visib", "bbox_obj", "bbox_visib", "mask_all", "mask_visib", "near_counts")
PH, PW = vo.PLATE_HW


@functools.lru_cache(maxsize=None)
def _mixed():
    """The twelve ground truths of the mixed scene (two images, three objects, uint16 depth), computed once and never modified."""
    ms = vo.mixed_scene()
    views = {"objects": ms["objects"], "obj_ids": ms["obj_ids"], "image_index": ms["image_index"], "R": ms["R_gt"], "t": ms["t_gt"],
             "cams": vo.CAMS, "depth": vo.depth_mm32(ms["depth_u16"], ms["depth_scale"])}
    return ms, views


@functools.lru_cache(maxsize=None)
def _mixed_ref(pad="bop", depth=True, delta=15.0):
    return so.scene_reference(_mixed()[1], vo.H, vo.W, pad, "scene" if depth else None, delta)


@functools.lru_cache(maxsize=None)
def _edge_ref():
    return so.scene_reference(so.edge_scene(), vo.H, vo.W)


def _run(models, scene, rows=None, depth="scene", hw=(vo.H, vo.W), **kw):
    rows = np.arange(len(scene["obj_ids"])) if rows is None else rows
    d = scene.get("depth") if isinstance(depth, str) else depth
    kw.setdefault("masks", "both")
    r = sg.scene_gt_info(models, scene["obj_ids"][rows], scene["R"][rows], scene["t"][rows], vo.k33(np.asarray(scene["cams"], dtype=F)),
                         depth=d, resolution=hw, image_index=scene["image_index"][rows], **kw)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _assert_equals_oracle(got, ref, rows=None):
    rows = np.arange(len(ref["counts"])) if rows is None else rows
    c = np.stack([got["px_count_all"], got["px_count_valid"], got["px_count_visib"]], axis=1)
    assert np.array_equal(c, ref["counts"][rows]), (c, ref["counts"][rows])
    assert np.array_equal(got["bbox_obj"], ref["bbox_obj"][rows]) and np.array_equal(got["bbox_visib"], ref["bbox_visib"][rows])
    assert got["mask_all"].dtype == np.uint8 and np.array_equal(got["mask_all"], ref["mask_all"][rows])
    assert np.array_equal(got["mask_visib"], ref["mask_visib"][rows])
    assert np.array_equal(got["near_counts"], ref["near"][rows]) and got["near_count"] == ref["near"][rows].sum()
    f = np.divide(ref["counts"][rows, 2], ref["counts"][rows, 0], out=np.zeros(len(rows)), where=ref["counts"][rows, 0] > 0)
    assert got["visib_fract"].dtype == np.float64 and np.array_equal(got["visib_fract"], f)


@gpu
def test_mixed_scene_equals_the_oracle_for_both_canvases_windows_and_groupings():
    ms, views = _mixed()
    models = ev.ObjectModels(views["objects"])
    depth = dict(depth=ms["depth_u16"], depth_scale=ms["depth_scale"])
    for pad in ((0, 0), "bop"):
        ref = _mixed_ref(pad)
        for window in ("auto", "full"):
            got = _run(models, views, pad=pad, window=window, **depth)
            _assert_equals_oracle(got, ref)
            assert got["n_groups"] == 1
        split = _run(models, views, pad=pad, workspace_bytes=40000, **depth)
        assert split["n_groups"] > 2
        _assert_equals_oracle(split, ref)
    assert ref["counts"][:, 2].tolist() == [183, 920, 157, 282, 240, 238, 92, 15, 44, 319, 128, 83]
    # tied to the existing kernels at pad (0, 0): the visible count is VSD's union of a pair whose estimate IS the ground truth, and the
    # covered samples are render_depth's
    got = _run(models, views, pad=(0, 0), **depth)
    vsd = ev.vsd_errors(models, ms["obj_ids"], ms["R_gt"], ms["t_gt"], ms["R_gt"], ms["t_gt"], ms["K"], ms["depth_u16"],
                        image_index=ms["image_index"], depth_scale=ms["depth_scale"])
    assert np.array_equal(vsd["visib_union"].cpu().numpy(), got["px_count_visib"])
    z = ev.render_depth(models, ms["obj_ids"], ms["R_gt"], ms["t_gt"], ms["K"], (vo.H, vo.W), image_index=ms["image_index"])["depth"]
    assert np.array_equal((z > 0).cpu().numpy(), got["mask_all"] == 255)
    _one_packed_scene_through_both_entries()


def _one_packed_scene_through_both_entries():
    """The same equality without the public functions between the two kernels: ONE scene.PackedScene, and the SAME PpScene instance,
    goes to pp_vsd_errors (depth_out only) and to pp_scene_gt (pad (0, 0), mask_all, a float depth of zeros).  48 x 64 frame; the
    12-triangle box and a tetrahedron (made here: the oracles' scenes hold none); four views: the box centred, the tetrahedron cut by
    the right frame edge (its window is clipped there), the box off-frame (an empty window) and a pose with a NaN (an empty window)."""
    H, W, K4 = 48, 64, (100.0, 100.0, 31.5, 23.5)
    box = ro.cube(40.0)
    tetra = {"vertices": np.array([[30, 30, 30], [30, -30, -30], [-30, 30, -30], [-30, -30, 30]], dtype=F),
             "faces": np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)}
    objects = {1: {"vertices": box["vertices"], "faces": box["faces"], "info": {"diameter": 140.0}},
               2: {"vertices": tetra["vertices"], "faces": tetra["faces"], "info": {"diameter": 85.0}}}
    models = ev.ObjectModels(objects)
    rng = np.random.default_rng(11)
    poses = np.stack([vo.pose(vo.random_rotation(rng), t) for t in ((0, 0, 400.0), (120.0, 10.0, 400.0), (2000.0, 0, 400.0), (0, 0, 400.0))]).astype(F)
    poses[3, 1, 1] = np.nan
    obj, img = np.array([0, 1, 0, 1], dtype=np.int32), np.zeros(4, dtype=np.int32)
    cams = np.array([K4], dtype=F)
    windows = scn.view_windows(models, obj, img, poses, cams, H, W, 1.0, "auto")
    assert 0 < windows[0, 0] and windows[0, 2] < W and windows[1, 2] == W and 0 < windows[1, 0] and not windows[2:].any()
    want = np.zeros((4, H, W), dtype=F)
    for v in (0, 1, 2):
        want[v] = vo.depth32(objects[int(obj[v]) + 1]["vertices"], objects[int(obj[v]) + 1]["faces"], poses[v], cams[0], H, W)[0]
    assert (want[0] > 0).sum() > 300 and (want[1][:, -1] > 0).any() and not (want[1][:, 0] > 0).any() and not want[2].any()

    packed = scn.PackedScene(models, cams, H, W, 1.0, obj, img, poses, windows)
    L, dev, need = _lib.lib(), models.device, ctypes.c_size_t()
    _lib.check(L.pp_vsd_workspace_bytes(packed.samples, packed.faces, ctypes.byref(need)), "pp_vsd_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)  # noqa: E731
    dense, near_vsd, near_gt, counts, boxes = torch.empty((4, H, W), dtype=torch.float32, device=dev), i32(4), i32(4), i32(4, 3), i32(4, 8)
    mask_all, zeros = torch.empty((4, H, W), dtype=torch.uint8, device=dev), torch.zeros((1, H, W), dtype=torch.float32, device=dev)
    tau = np.zeros(1, dtype=F)
    sc = ctypes.byref(packed.scene)
    _lib.check(L.pp_vsd_errors(sc, None, None, None, None, 0, None, 15.0, tau.ctypes.data, 1, ws.data_ptr(), ws.numel(), None, None,
                               near_vsd.data_ptr(), dense.data_ptr(), _lib.stream_ptr()), "pp_vsd_errors")
    # pad (0, 0): the canvas cameras are the frame cameras, so the scene's own tables serve as both
    _lib.check(L.pp_scene_gt(sc, packed.scene.cams, packed.scene.cams_host, 0, 0, zeros.data_ptr(), 15.0, None, 0, ws.data_ptr(), ws.numel(),
                             counts.data_ptr(), boxes.data_ptr(), near_gt.data_ptr(), mask_all.data_ptr(), None, None, None,
                             _lib.stream_ptr()), "pp_scene_gt")
    torch.cuda.synchronize()
    z, m, c = dense.cpu().numpy(), mask_all.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(z.view(np.int32), want.view(np.int32))
    assert m.dtype == np.uint8 and np.array_equal(m, 255 * (z > 0).astype(np.uint8)) and np.array_equal(m, 255 * (want > 0).astype(np.uint8))
    assert np.array_equal(c[:, 0], (z > 0).reshape(4, -1).sum(axis=1)) and np.array_equal(c[:, 0], (want > 0).reshape(4, -1).sum(axis=1))
    assert c[2:].tolist() == [[0, 0, 0]] * 2 and not near_vsd.cpu().numpy().any() and not near_gt.cpu().numpy().any()


@gpu
def test_edge_scene_plate_rows_and_a_nan_pose():
    """The whole-canvas window (the camera inside the sphere: 9 H W samples, near-plane drops), instances over every border, one off the
    frame but on the canvas, one behind the camera, missing depth, and a NaN pose, which renders nothing."""
    scene = so.edge_scene()
    models = ev.ObjectModels(scene["objects"])
    ref = _edge_ref()
    got = _run(models, scene)
    _assert_equals_oracle(got, ref)
    assert got["px_count_all"].tolist() == [468, 467, 409, 394, 97200, 256, 0, 293, 271] and got["near_counts"].tolist() == [0, 0, 0, 0, 184, 0, 12, 0, 0]
    assert got["px_count_visib"].tolist() == [123, 265, 238, 101, 10800, 0, 0, 293, 184]
    assert got["bbox_visib"][5].tolist() == [0, 0, -1, -1] == got["bbox_obj"][6].tolist()
    bad = dict(scene, t=scene["t"].copy())
    bad["t"][7, 1] = np.nan
    nan = _run(models, bad)
    assert [int(nan[k][7]) for k in KEYS[:3]] == [0, 0, 0] and nan["bbox_obj"][7].tolist() == [0, 0, -1, -1] == nan["bbox_visib"][7].tolist()
    assert nan["mask_all"][7].max() == 0 and nan["visib_fract"][7] == 0
    keep = np.arange(9) != 7
    for k in KEYS:
        assert np.array_equal(nan[k][keep], got[k][keep]), k
    # the plate rows: closed forms through the kernel
    rows = [((0, 0, 500), 256, (33, 23, 48, 38), (33, 23, 48, 38)), ((-200, 0, 500), 144, (-7, 23, 8, 38), (0, 23, 8, 38)),
            ((-200, -150, 500), 81, (-7, -7, 8, 8), (0, 0, 8, 8)), ((235, 180, 500), 6, (80, 59, 95, 74), (80, 59, 82, 60)),
            ((-400, 0, 500), 0, (-47, 23, -32, 38), (0, 0, -1, -1))]
    plates = dict(so.plate_scene([r[0] for r in rows]), depth=np.zeros((1, PH, PW), dtype=F))
    pm = ev.ObjectModels(plates["objects"])
    p = _run(pm, plates, hw=(PH, PW), pad=(83, 61))
    _assert_equals_oracle(p, so.scene_reference(plates, PH, PW, (83, 61)))
    for k, (_, inframe, bo, bv) in enumerate(rows):
        assert (p["px_count_all"][k], p["px_count_valid"][k], p["px_count_visib"][k]) == (256, 0, inframe)
        assert tuple(p["bbox_obj"][k]) == bo and tuple(p["bbox_visib"][k]) == bv
    assert p["visib_fract"].tolist() == [1.0, 0.5625, 81 / 256, 6 / 256, 0.0]
    p0 = _run(pm, plates, hw=(PH, PW), pad=(0, 0))
    assert p0["px_count_all"].tolist() == [256, 144, 81, 6, 0] and np.array_equal(p0["bbox_obj"], p0["bbox_visib"])
    occ = _run(pm, so.plate_scene([(0, 0, 500)]), depth=vo.plate_cases()["occluder"][2][None], hw=(PH, PW))
    assert (occ["px_count_all"][0], occ["px_count_valid"][0], occ["px_count_visib"][0]) == (256, 128, 128) and tuple(occ["bbox_visib"][0]) == (41, 23, 48, 38)


@gpu
def test_composite_visibility_scene_depth_and_instance_map():
    two = so.plate_scene([(0, 0, 400), (60, 0, 500)])
    pm = ev.ObjectModels(two["objects"])
    for delta, visib in ((0.0, 160), (15.0, 160), (150.0, 256)):
        r = _run(pm, two, depth=None, hw=(PH, PW), delta=delta, composite=True)
        assert r["px_count_all"].tolist() == [400, 256] == r["px_count_valid"].tolist() and r["px_count_visib"].tolist() == [400, visib]
        assert r["bbox_obj"].tolist() == [[31, 21, 50, 40], [45, 23, 60, 38]]
        _assert_equals_oracle(r, so.scene_reference(two, PH, PW, "bop", None, delta))
    same = _run(pm, so.plate_scene([(0, 0, 500), (0, 0, 500)]), depth=None, hw=(PH, PW), delta=0.0, composite=True)
    assert set(np.unique(same["instance_map"])) == {-1, 0} and same["px_count_visib"].tolist() == [256, 256]      # a tie: the lower index
    ms, views = _mixed()
    models = ev.ObjectModels(views["objects"])
    want = {0.0: [183, 920, 305, 598, 240, 238, 159, 176, 44, 310, 281, 92], 15.0: [185, 920, 305, 609, 240, 238, 159, 176, 44, 320, 281, 92]}
    for delta in (0.0, 15.0):
        ref = _mixed_ref("bop", False, delta)
        for kw in ({}, {"workspace_bytes": 200000}):
            r = _run(models, views, depth=None, delta=delta, composite=True, **kw)
            assert r["n_groups"] == (2 if kw else 1)
            _assert_equals_oracle(r, ref)
            assert r["px_count_visib"].tolist() == want[delta]
            assert r["scene_depth"].dtype == F and np.array_equal(r["scene_depth"].view(np.int32), ref["scene_depth"].view(np.int32))
            assert r["instance_map"].dtype == np.int32 and np.array_equal(r["instance_map"], ref["instance_map"])
    assert len(np.unique(ref["instance_map"])) == 13
    # composite asked for together with a depth image: the counts stay the depth-mode ones, the composite is the same
    both = _run(models, views, depth=ms["depth_u16"], depth_scale=ms["depth_scale"], composite=True)
    _assert_equals_oracle(both, _mixed_ref("bop"))
    assert np.array_equal(both["scene_depth"].view(np.int32), ref["scene_depth"].view(np.int32)) and np.array_equal(both["instance_map"], ref["instance_map"])
    with pytest.raises(ValueError, match="image"):
        _run(models, views, depth=None, workspace_bytes=100000)


@gpu
def test_results_do_not_depend_on_view_order_stream_or_grouping():
    ms, views = _mixed()
    models = ev.ObjectModels(views["objects"])
    n = len(views["obj_ids"])
    perm = np.random.default_rng(0).permutation(n)
    inv = np.argsort(perm)
    for mode in ({"depth": ms["depth_u16"], "depth_scale": ms["depth_scale"], "workspace_bytes": 1},
                 {"depth": None, "delta": 0.0, "workspace_bytes": 200000}):
        small = mode.pop("workspace_bytes")
        base = _run(models, views, composite=True, **mode)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = _run(models, views, composite=True, **mode)
        side.synchronize()
        shuffled = _run(models, views, rows=perm, composite=True, **mode)
        grouped = _run(models, views, composite=True, workspace_bytes=small, **mode) if mode["depth"] is None else \
            _run(models, views, workspace_bytes=small, **mode)
        assert base["n_groups"] == 1 and grouped["n_groups"] == (2 if mode["depth"] is None else n)
        for k in KEYS:
            assert base[k].tobytes() == other[k].tobytes() == grouped[k].tobytes() and base[k][perm].tobytes() == shuffled[k].tobytes(), k
        assert base["visib_fract"].tobytes() == other["visib_fract"].tobytes() == shuffled["visib_fract"][inv].tobytes()
        assert base["scene_depth"].tobytes() == other["scene_depth"].tobytes() == shuffled["scene_depth"].tobytes()
        relabelled = np.where(shuffled["instance_map"] >= 0, perm[np.maximum(shuffled["instance_map"], 0)], -1)
        assert np.array_equal(base["instance_map"], other["instance_map"]) and np.array_equal(base["instance_map"], relabelled)
        if mode["depth"] is None:
            assert base["scene_depth"].tobytes() == grouped["scene_depth"].tobytes() and np.array_equal(base["instance_map"], grouped["instance_map"])


@gpu
def test_no_views_no_launch():
    ms, views = _mixed()
    models = ev.ObjectModels(views["objects"])
    r = _run(models, views, rows=np.zeros(0, dtype=np.int64), composite=True)
    assert r["px_count_all"].shape == (0,) and r["bbox_obj"].shape == (0, 4) and r["mask_visib"].shape == (0, vo.H, vo.W) and r["n_groups"] == 0
    assert r["scene_depth"].shape == (2, vo.H, vo.W) and r["scene_depth"].max() == 0 and r["instance_map"].max() == -1


def _one_image():
    """A 90 x 120 image: a cube, a sphere, and a second sphere behind an occluder that hides all but its right edge (below 10 %)."""
    objs = {o: v for o, v in vo.objects().items() if o != 3}
    rng = np.random.default_rng(8)
    inst = [(1, vo.random_rotation(rng), (-110.0, -20, 520)), (2, np.eye(3), (10.0, 15, 500)), (2, np.eye(3), (140.0, -30, 560))]
    depth = np.full((vo.H, vo.W), 1500.0, dtype=F)
    hits = []
    for o, R, t in inst:
        z, _ = vo.depth32(objs[o]["vertices"], objs[o]["faces"], vo.pose(R, t), vo.CAMS[0], vo.H, vo.W)
        depth = np.where(z > 0, np.minimum(depth, np.where(z > 0, z, np.inf)), depth)
        hits.append(z > 0)
    xs = np.where(hits[2].any(axis=0))[0]
    depth[:, xs.min():xs.max()] = np.minimum(depth[:, xs.min():xs.max()], 300.0)       # everything but the last column of the instance
    gt = {4: {7: {"obj_id": np.array([i[0] for i in inst]), "R": np.stack([F(i[1]) for i in inst]).astype(np.float64),
                  "t": np.stack([F(i[2]) for i in inst]).astype(np.float64)}}}
    cams = {4: {7: {"K": vo.k33(vo.CAMS[:1])[0].astype(np.float64), "depth_scale": 0.5}}}
    return objs, gt, cams, np.rint(depth / 0.5).astype(np.uint16)


@gpu
def test_end_to_end_detections_targets_and_scoring_from_ground_truth():
    objs, gt, cams, raw = _one_image()
    models = ev.ObjectModels(objs)
    g = gt[4][7]
    # ablation: ground-truth masks as detection records, through the detection batch
    r = sg.scene_gt_info(models, g["obj_id"], g["R"], g["t"], cams[4][7]["K"], depth=raw[None], depth_scale=0.5, masks="visib")
    dense = r["mask_visib"].cpu().numpy()
    dets = sg.gt_detections(g["obj_id"], r, scene_id=4, im_id=7)
    assert len(dets) == 3 and [d["category_id"] for d in dets] == [1, 2, 2]
    image = np.random.default_rng(1).integers(0, 256, size=(vo.H, vo.W, 3), dtype=np.uint8)
    idx = {1: 0, 2: 1}
    data = tb.assemble_test_image(image, dets, cams[4][7]["K"].ravel(), idx, scene_id=4, img_id=7)
    indep = tb.assemble_test_image(image, [do.record(m > 0, 1.0, o, time=0.0, compressed=False) for m, o in zip(dense, g["obj_id"])],
                                   cams[4][7]["K"].ravel(), idx, scene_id=4, img_id=7)
    for k in ("real_mask", "real_rgb", "real_bbox", "real_M", "obj_id", "score"):
        assert torch.equal(data[k], indep[k]), k
    boxes = data["real_bbox"].cpu().numpy()[0]
    for k in range(2):                                            # (the third mask has too few pixels: its window comes from the box)
        assert boxes[k].tolist() == [float(v) for v in get_bbox(dense[k])] and do.decode(dets[k]["segmentation"]).sum() * 255 == dense[k].sum(dtype=np.int64)
    ys, xs = np.where(dense[2])
    assert dets[2]["bbox"] == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1] and float(data["real_mask"][0, 0].max()) == 1.0
    # scoring: info -> targets -> the localisation protocol with the ground-truth poses as estimates
    info = sg.dataset_gt_info(gt, cams, models, (vo.H, vo.W), depth_images={4: {7: raw}})
    fr = [e["visib_fract"] for e in info[4][7]]
    assert fr[0] > 0.9 and fr[1] > 0.9 and 0 < fr[2] < 0.1 and info[4][7] == sg.format_gt_info(sg.scene_gt_info(
        models, g["obj_id"], g["R"], g["t"], cams[4][7]["K"], depth=raw[None], depth_scale=0.5))
    targets = sg.targets_from_gt_info(gt, info)
    assert targets.tolist() == [[4, 7, 1, 1], [4, 7, 2, 1]]        # the hidden sphere is no target
    est = {"scene_id": np.full(3, 4), "im_id": np.full(3, 7), "obj_id": g["obj_id"], "score": np.array([0.9, 0.8, 0.1]), "R": g["R"], "t": g["t"],
           "time": np.zeros(3)}
    res = ev.match_and_score(est, gt, targets, models, cams, image_width=vo.W, depth_images={4: {7: raw}})
    assert res["n_targets"] == 2 and res["AR_MSSD"] == 1.0 and res["AR_MSPD"] == 1.0 and res["AR_VSD"] == 1.0 and res["AR"] == 1.0
    # composite visibility (no depth images): nothing but the instances themselves hides anything
    free = sg.dataset_gt_info(gt, cams, models, (vo.H, vo.W), images_per_call=1)
    assert [e["visib_fract"] for e in free[4][7]] == [1.0, 1.0, 1.0] and sg.targets_from_gt_info(gt, free).tolist() == [[4, 7, 1, 1], [4, 7, 2, 2]]
