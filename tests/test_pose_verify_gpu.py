"""GPU: pp_pose_verify (picopose_amd/verify.py) against tests/verify_oracle.py: the counts equal to the float32 restatement bit for bit
and the mask areas equal to the decoder's on the mixed scene (with and without depth), on a 45 x 70 frame whose columns straddle
mask words, on a 96 x 80 frame sampled in full so that several workgroups add into one view, with empty and full masks, off-frame
and NaN poses and a depth image holding 0 and NaN; determinism across view order, grouping, window and stream; the tie to
render_depth and scene_gt_info; and verify_predictions end to end."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_oracle as vfo  # noqa: E402
import vsd_oracle as vo  # noqa: E402

from picopose_amd import _lib  # noqa: E402
from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import pipeline as pl  # noqa: E402
from picopose_amd import scene as scn  # noqa: E402
from picopose_amd import scene_gt as sg  # noqa: E402
from picopose_amd import verify as vf  # noqa: E402  (absent before the feature: every test here fails without it)
from picopose_amd.masks import RunTable, rle_counts, run_ends  # noqa: E402

gpu = pytest.mark.gpu
F = np.float32
TENSORS = ("counts", "mask_area", "iou", "visible_iou", "agreement", "score")
HYPS = 4


@functools.lru_cache(maxsize=None)
def _mixed():
    """The oracles' mixed scene (three objects, two images, uint16 depth): each of the twelve ground-truth views has four perturbed
    hypotheses, which share the mask decoded from the ground-truth render.  Computed once and never modified."""
    ms = vo.mixed_scene()
    rng = np.random.default_rng(5)
    n = len(ms["obj_ids"])
    segs, masks, R, t = [], [], [], []
    for g in range(n):
        o = ms["objects"][int(ms["obj_ids"][g])]
        z, _ = vo.depth32(o["vertices"], o["faces"], vo.pose(ms["R_gt"][g], ms["t_gt"][g]), vo.CAMS[ms["image_index"][g]], vo.H, vo.W)
        segs.append(vfo.rle(z > 0))
        masks.append(vfo.decode(segs[-1]))
        for _ in range(HYPS):
            R.append((ms["R_gt"][g].astype(np.float64) @ vo.random_rotation(rng, rng.uniform(0, 0.15))).astype(F))
            t.append((ms["t_gt"][g] + rng.normal(size=3) * [8.0, 8.0, 25.0]).astype(F))
    scene = {"objects": ms["objects"], "obj_ids": np.repeat(ms["obj_ids"], HYPS), "image_index": np.repeat(ms["image_index"], HYPS),
             "R": np.stack(R), "t": np.stack(t), "cams": vo.CAMS, "hw": (vo.H, vo.W), "segs": segs, "masks": masks,
             "mask_index": np.repeat(np.arange(n), HYPS), "depth": vo.depth_mm32(ms["depth_u16"], ms["depth_scale"]),
             "depth_arg": {"depth": ms["depth_u16"], "depth_scale": ms["depth_scale"]}}
    return scene


def _small(H, W, seed):
    """A frame of any size under one camera: the cube and the sphere over the middle, the corners and the borders, one view off the
    frame and one with a NaN; masks: a block that touches the last pixel, the frame's border ring, an empty and a full one, a band;
    a depth image with a wall, a near band (occluding), a far band (seen through), zeros and NaNs."""
    rng = np.random.default_rng(seed)
    objs = {o: v for o, v in vo.objects().items() if o != 3}
    cam = np.array([[100.0, 100.0, (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.25]], dtype=F)
    ex, ey = (W / 2) * 5.0, (H / 2) * 5.0                          # millimetres from the axis to the frame's edge at Z = 500
    spots = [(0, 0, 500), (ex - 5, ey - 5, 500), (-ex, 0, 520), (0, -ey, 480), (ex * 0.4, ey * 0.3, 450), (-ex * 0.5, ey * 0.6, 560)]
    ring = np.ones((H, W), dtype=bool)
    ring[1:-1, 1:-1] = False
    block = np.zeros((H, W), dtype=bool)
    block[H - H // 3:, W - W // 3:] = True                         # reaches the last pixel (x, y) = (W - 1, H - 1)
    band = np.zeros((H, W), dtype=bool)
    band[:, W // 4:W // 4 + W // 2] = True
    masks = [block, ring, np.zeros((H, W), dtype=bool), np.ones((H, W), dtype=bool), band]
    obj, R, t, midx = [], [], [], []
    for k, s in enumerate(spots):
        for m in range(len(masks)):
            obj.append(1 + (k + m) % 2)
            R.append(vo.random_rotation(rng).astype(F))
            t.append(F(s))
            midx.append(m)
    for s in ((5000.0, 0.0, 500.0), (0.0, 0.0, 500.0)):           # off the frame, and (below) a NaN
        obj.append(2), R.append(np.eye(3, dtype=F)), t.append(F(s)), midx.append(3)
    t[-1][1] = np.nan
    depth = np.full((1, H, W), 530.0, dtype=F)
    depth[0, :, : W // 5], depth[0, :, W - W // 5:] = 300.0, 900.0
    depth[0, H // 2 - 3:H // 2 + 3, W // 3:W // 2], depth[0, H // 3:H // 2, W // 2:W // 2 + 6] = 0.0, np.nan
    return {"objects": objs, "obj_ids": np.array(obj), "image_index": np.zeros(len(obj), dtype=np.int32), "R": np.stack(R), "t": np.stack(t),
            "cams": cam, "hw": (H, W), "segs": [vfo.rle(m) for m in masks], "masks": masks, "mask_index": np.array(midx), "depth": depth,
            "depth_arg": {"depth": depth}}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return {"mixed": _mixed, "45x70": lambda: _small(45, 70, 1), "96x80": lambda: _small(96, 80, 2)}[name]()


@functools.lru_cache(maxsize=None)
def _ref(name, depth):
    s = _scene(name)
    poses = [vo.pose(R, t) for R, t in zip(s["R"], s["t"])]
    return vfo.reference(s["objects"], s["obj_ids"], poses, s["image_index"], s["cams"], *s["hw"], s["masks"], s["mask_index"],
                         s["depth"] if depth else None)


def _run(models, s, depth, rows=None, **kw):
    rows = np.arange(len(s["obj_ids"])) if rows is None else rows
    r = vf.verify_poses(models, s["obj_ids"][rows], s["R"][rows], s["t"][rows], vo.k33(np.asarray(s["cams"], dtype=F)), s["segs"], s["hw"],
                        mask_index=s["mask_index"][rows], image_index=s["image_index"][rows], **(s["depth_arg"] if depth else {}), **kw)
    assert all(r[k].is_cuda for k in TENSORS)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _assert_equals_oracle(got, ref, s, depth):
    assert got["counts"].dtype == np.int32 and got["counts"].shape == ref["counts"].shape
    assert np.array_equal(got["counts"], ref["counts"]), np.argwhere(got["counts"] != ref["counts"])
    assert got["mask_area"].dtype == np.int32 and np.array_equal(got["mask_area"], ref["mask_area"])
    assert got["near_count"] == ref["near"].sum()
    want = vfo.scores(ref["counts"], ref["mask_area"][s["mask_index"]], depth)
    for k, w in zip(("iou", "visible_iou", "agreement", "score"), want):
        assert got[k].dtype == np.float64 and np.array_equal(got[k], w), k


@gpu
@pytest.mark.parametrize("depth", (True, False), ids=("depth", "rgb"))
def test_mixed_scene_equals_the_oracle(depth):
    s, ref = _scene("mixed"), _ref("mixed", depth)
    models = ev.ObjectModels(s["objects"])
    got = _run(models, s, depth)
    _assert_equals_oracle(got, ref, s, depth)
    assert got["n_groups"] == 1 and len(s["obj_ids"]) == 48
    c = ref["counts"]
    # conditions of the test, on the oracle alone: every counter is exercised, and float32 decides every sample as float64 does
    assert np.array_equal(c, ref["counts64"]) and (c[:, 1] > 0).sum() >= 40
    if depth:
        assert all((c[:, k] > 0).any() for k in range(8)) and (c[:, 6] < c[:, 0]).any()
    else:
        assert not c[:, 2:6].any() and np.array_equal(c[:, 6:], c[:, :2])


@gpu
@pytest.mark.parametrize("name,window", (("45x70", "auto"), ("45x70", "full"), ("96x80", "full"), ("96x80", "auto")))
def test_small_frames_masks_poses_and_depth_holes_equal_the_oracle(name, window):
    """45 x 70: H is no multiple of 32, so a column's bits straddle mask words, and H W = 3150 is none either, so the last word is
    partial; a mask reaches the last pixel.  96 x 80 in full: 7680 window samples, more than the 4096 a workgroup owns per chunk, so
    two workgroups add into each view.  Empty and full masks, an off-frame view and a NaN pose (zero counts), depth holding 0 and NaN."""
    s = _scene(name)
    models = ev.ObjectModels(s["objects"])
    H, W = s["hw"]
    assert s["masks"][0][H - 1, W - 1] and s["masks"][1][0].all() and not s["masks"][2].any() and s["masks"][3].all()
    assert np.isnan(s["depth"]).any() and (s["depth"] == 0).any()
    for depth in (True, False):
        ref = _ref(name, depth)
        got = _run(models, s, depth, window=window)
        _assert_equals_oracle(got, ref, s, depth)
        assert not got["counts"][-2:].any() and got["score"][-2:].tolist() == [0.0, 0.0]       # off the frame; NaN
        c = ref["counts"]
        assert np.array_equal(c, ref["counts64"])
        assert not c[s["mask_index"] == 2, 1].any() and np.array_equal(c[s["mask_index"] == 3, 1], c[s["mask_index"] == 3, 0])
        assert (c[s["mask_index"] == 0, 1] > 0).any() and (c[s["mask_index"] == 1, 1] > 0).any()
        if depth:
            assert (c[:, 2] < c[:, 0]).any() and (c[:, 4] > 0).any() and (c[:, 5] > 0).any() and (c[:, 3] > 0).any()
    if name == "96x80":
        assert H * W > 4096


@gpu
@pytest.mark.parametrize("name,window", (("45x70", "auto"), ("96x80", "full")))
def test_the_entry_through_the_abi_clears_its_outputs_and_equals_the_oracle(name, window):
    """pp_pose_verify itself on ONE scene.PackedScene, without verify_poses between the test and the kernel: counts and near_count are
    filled with -7 before each call (the entry clears them; the reduction only adds), with and without the depth image."""
    s, ref = _scene(name), _ref(name, True)
    models = ev.ObjectModels(s["objects"])
    dev, (H, W), n = models.device, s["hw"], len(s["obj_ids"])
    obj = scn.obj_index(models, s["obj_ids"])
    poses = scn.pose44(s["R"], s["t"])
    cams = np.asarray(s["cams"], dtype=F)
    windows = scn.view_windows(models, obj, s["image_index"], poses, cams, H, W, 1.0, window)
    packed = scn.PackedScene(models, cams, H, W, 1.0, obj, s["image_index"], poses, windows)
    L, need = _lib.lib(), ctypes.c_size_t()
    _lib.check(L.pp_vsd_workspace_bytes(packed.samples, packed.faces, ctypes.byref(need)), "pp_vsd_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    bits, area = RunTable.upload([run_ends(rle_counts(seg, size=(H, W))) for seg in s["segs"]], dev).pack(H * W)
    vm = np.ascontiguousarray(s["mask_index"], dtype=np.int32)
    vm_d = torch.from_numpy(vm).to(dev)
    depth = torch.from_numpy(np.ascontiguousarray(s["depth"], dtype=F)).to(dev)
    for with_depth in (True, False):
        want = ref["counts"] if with_depth else _ref(name, False)["counts"]
        counts = torch.full((n, 8), -7, dtype=torch.int32, device=dev)
        near = torch.full((n,), -7, dtype=torch.int32, device=dev)
        _lib.check(L.pp_pose_verify(ctypes.byref(packed.scene), bits.data_ptr(), len(s["segs"]), bits.shape[1], vm_d.data_ptr(),
                                    vm.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), depth.data_ptr() if with_depth else None, 15.0,
                                    ws.data_ptr(), ws.numel(), counts.data_ptr(), near.data_ptr(), _lib.stream_ptr()), "pp_pose_verify")
        assert np.array_equal(counts.cpu().numpy(), want), with_depth
        assert np.array_equal(near.cpu().numpy(), ref["near"])
    assert np.array_equal(area.cpu().numpy(), ref["mask_area"])


@gpu
def test_results_do_not_depend_on_view_order_grouping_window_or_stream():
    s = _scene("mixed")
    models = ev.ObjectModels(s["objects"])
    n = len(s["obj_ids"])
    perm = np.random.default_rng(0).permutation(n)
    for depth in (True, False):
        base = _run(models, s, depth)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = _run(models, s, depth)
        side.synchronize()
        shuffled = _run(models, s, depth, rows=perm)
        grouped = _run(models, s, depth, workspace_bytes=1)
        some = _run(models, s, depth, workspace_bytes=60000)
        full = _run(models, s, depth, window="full")
        assert base["n_groups"] == 1 and grouped["n_groups"] == n and 2 < some["n_groups"] < n
        for k in TENSORS:
            assert base[k].tobytes() == other[k].tobytes() == grouped[k].tobytes() == some[k].tobytes() == full[k].tobytes(), k
            if k != "mask_area":
                assert base[k][perm].tobytes() == shuffled[k].tobytes(), k
        assert base["near_count"] == other["near_count"] == grouped["near_count"] == shuffled["near_count"] == full["near_count"]


@gpu
def test_tied_to_render_depth_and_scene_gt_info():
    """The mask equal to the ground-truth render's own silhouette: without depth render == inter == A (iou 1); with depth `vis` is
    scene_gt_info(pad=(0, 0))'s px_count_visib of the same view."""
    ms = vo.mixed_scene()
    models = ev.ObjectModels(ms["objects"])
    z = ev.render_depth(models, ms["obj_ids"], ms["R_gt"], ms["t_gt"], ms["K"], (vo.H, vo.W), image_index=ms["image_index"])["depth"]
    segs = [sg.rle_from_mask(m) for m in (z > 0).cpu().numpy()]
    args = (models, ms["obj_ids"], ms["R_gt"], ms["t_gt"], ms["K"], segs, (vo.H, vo.W))
    rgb = vf.verify_poses(*args, image_index=ms["image_index"])
    c, area = rgb["counts"].cpu().numpy(), rgb["mask_area"].cpu().numpy()
    assert (area > 0).all() and np.array_equal(c[:, 0], area) and np.array_equal(c[:, 1], area) and np.array_equal(c[:, 6:], c[:, :2])
    assert rgb["iou"].cpu().tolist() == [1.0] * 12 == rgb["score"].cpu().tolist()
    with_depth = vf.verify_poses(*args, image_index=ms["image_index"], depth=ms["depth_u16"], depth_scale=ms["depth_scale"])
    info = sg.scene_gt_info(models, ms["obj_ids"], ms["R_gt"], ms["t_gt"], ms["K"], depth=ms["depth_u16"], depth_scale=ms["depth_scale"],
                            image_index=ms["image_index"], pad=(0, 0))
    d = with_depth["counts"].cpu().numpy()
    assert np.array_equal(d[:, 6], info["px_count_visib"].cpu().numpy()) and np.array_equal(d[:, 2], info["px_count_valid"].cpu().numpy())
    assert np.array_equal(d[:, 0], info["px_count_all"].cpu().numpy()) and np.array_equal(d[:, 7], d[:, 6])
    assert d[:, 6].tolist() == [183, 920, 157, 282, 240, 238, 92, 15, 44, 319, 128, 83]


@functools.lru_cache(maxsize=None)
def _one_image():
    """A 90 x 120 image: a cube, a sphere and a second sphere whose left third an occluder hides; per instance three hypotheses, the
    ground truth in the MIDDLE (the inlier-ratio order has it second) between two that are shifted and rotated."""
    objs = {o: v for o, v in vo.objects().items() if o != 3}
    rng = np.random.default_rng(8)
    inst = [(1, vo.random_rotation(rng), (-110.0, -20, 520)), (2, np.eye(3), (10.0, 15, 500)), (2, np.eye(3), (120.0, -30, 560))]
    depth = np.full((vo.H, vo.W), 1500.0, dtype=F)
    for k, (o, R, t) in enumerate(inst):
        z, _ = vo.depth32(objs[o]["vertices"], objs[o]["faces"], vo.pose(R, t), vo.CAMS[0], vo.H, vo.W)
        depth = np.where(z > 0, np.minimum(depth, np.where(z > 0, z, np.inf)), depth).astype(F)
        if k == 2:
            xs = np.where((z > 0).any(axis=0))[0]
            depth[:, xs.min():xs.min() + (xs.max() - xs.min()) // 3] = 300.0
    preds = []
    for o, R, t in inst:
        hyps = []
        for ratio, angle, shift in ((0.9, 0.4, (-40.0, 25.0, 0.0)), (0.8, 0.0, (0.0, 0.0, 0.0)), (0.7, 0.8, (30.0, -35.0, 40.0))):
            Rh = np.asarray(R, dtype=np.float64) @ vo.random_rotation(rng, angle)
            hyps.append({"inliers_ratio": ratio, "R_stage_3": Rh.astype(F).ravel(), "t_stage_3": (np.asarray(t) + shift).astype(F)})
        preds.append(hyps)
    return objs, inst, depth, preds


@gpu
def test_verify_predictions_puts_the_ground_truth_first_and_bop_csv_lines_prints_it():
    objs, inst, depth, preds = _one_image()
    models = ev.ObjectModels(objs)
    ids = [i[0] for i in inst]
    K = vo.k33(vo.CAMS[:1])[0]
    gt_R, gt_t = np.stack([F(i[1]) for i in inst]), np.stack([F(i[2]) for i in inst])
    info = sg.scene_gt_info(models, ids, gt_R, gt_t, K, depth=depth[None], masks="visib")
    dets = sg.gt_detections(ids, info, scene_id=4, im_id=7)          # the detection records of the VISIBLE (modal) masks
    segs = [d["segmentation"] for d in dets]
    assert len(segs) == 3 and info["visib_fract"][2] < 0.8 < info["visib_fract"][0]
    for kw in ({"depth": depth}, {}):
        out = pl.verify_predictions(preds, models, ids, K, segs, (vo.H, vo.W), **kw)
        for k, hyps in enumerate(out):
            assert [h["inliers_ratio"] for h in hyps][0] == 0.8, (k, [(h["inliers_ratio"], h["verify_score"]) for h in hyps])
            assert hyps[0]["verify_score"] > hyps[1]["verify_score"] >= hyps[2]["verify_score"]
            assert hyps[0]["verify_counts"][0] > 0 and len(hyps[0]["verify_counts"]) == 8
            if kw:                                                  # the ground truth explains its visible mask exactly
                assert hyps[0]["verify_visible_iou"] == 1.0 and hyps[0]["verify_agreement"] == 1.0 == hyps[0]["verify_score"]
        assert [h["inliers_ratio"] for h in preds[0]] == [0.9, 0.8, 0.7] and "verify_score" not in preds[0][0]
        lines = pl.bop_csv_lines(4, 7, ids, [1.0] * 3, out, 0.0)
        for k, line in enumerate(lines):
            assert line.split(",")[5] == " ".join(str(v) for v in gt_t[k]) and line.split(",")[4] == " ".join(str(v) for v in gt_R[k].ravel())
    # hypotheses="best" verifies the first hypothesis only and keeps the order
    best = pl.verify_predictions(preds, models, ids, K, segs, (vo.H, vo.W), depth=depth, hypotheses="best", rank=False)
    assert all("verify_score" in h[0] and "verify_score" not in h[1] for h in best) and [h["inliers_ratio"] for h in best[1]] == [0.9, 0.8, 0.7]


@gpu
def test_no_poses_no_launch():
    s = _scene("45x70")
    models = ev.ObjectModels(s["objects"])
    r = _run(models, s, True, rows=np.zeros(0, dtype=np.int64))
    assert r["counts"].shape == (0, 8) and r["score"].shape == (0,) and r["n_groups"] == 0
    assert np.array_equal(r["mask_area"], [int(m.sum()) for m in s["masks"]])
