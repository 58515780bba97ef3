"""CPU: the pose-verification oracle (tests/verify_oracle.py) against closed forms on the plate that do not come from it, the score
formulas at their zero denominators, the argument checks of pp_pose_verify through the ABI (no GPU), every ValueError of
verify.verify_poses and pipeline.verify_predictions that precedes device work, and the rank=True ordering with verify_poses replaced."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_tables as st  # noqa: E402
import verify_oracle as vfo  # noqa: E402
import vsd_oracle as vo  # noqa: E402

from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import pipeline as pl  # noqa: E402
from picopose_amd import verify as vf  # noqa: E402  (absent before the feature: every test here fails without it)

F = np.float32
PH, PW = vo.PLATE_HW
DELTA = 15.0


def _rect(x0, x1, y0, y1, hw=(PH, PW)):
    """The mask of columns x0 .. x1 and rows y0 .. y1, inclusive."""
    m = np.zeros(hw, dtype=bool)
    m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def _plate_render(t):
    p = vo.plate(vo.PLATE_N)
    return vo.depth32(p["vertices"], p["faces"], vo.pose(t=t), vo.PLATE_K4, PH, PW)[0]


# The 16 x 16-sample plate at 500 mm under f = 100, principal point (40.5, 30.5): columns 33 .. 48, rows 23 .. 38; moved by
# (+50, -25) mm it covers columns 43 .. 58, rows 18 .. 33.  r = sqrt(xr^2 + yr^2 + 1) is below 1.03 over both, so a depth offset of
# `off` mm gives |e| = |off| r: 0, 5 and 14 stay below delta = 15 (14 * 1.03 < 15), 16 and 40 exceed it, with at least 0.5 mm to spare.
PLATES = [((0.0, 0.0, 500.0), (33, 48, 23, 38)), ((50.0, -25.0, 500.0), (43, 58, 18, 33))]
MASKS = [(30, 40, 20, 30), (0, PW - 1, 0, PH - 1), (45, 60, 30, 45), (0, 5, 0, 5)]


def _overlap(a, b):
    w, h = min(a[1], b[1]) - max(a[0], b[0]) + 1, min(a[3], b[3]) - max(a[2], b[2]) + 1
    return max(w, 0) * max(h, 0)


def test_plate_offsets_closed_forms_float32_equals_float64():
    for t, cover in PLATES:
        z = _plate_render(t)
        assert (z > 0).sum() == 256 and _overlap(cover, cover) == 256
        for rect in MASKS:
            mask, inter = _rect(*rect), _overlap(cover, rect)
            for off in (0.0, 5.0, -5.0, 14.0, -14.0, 16.0, -16.0, 40.0, -40.0):
                depth = np.full((PH, PW), t[2] + off, dtype=F)
                if abs(off) < DELTA:
                    want = [256, inter, 256, 256, 0, 0, 256, inter]
                elif off > 0:                                       # the sensor sees further than the model: it sees through it
                    want = [256, inter, 256, 0, 0, 256, 256, inter]
                else:                                               # the scene is closer: the model is occluded, nothing is visible
                    want = [256, inter, 256, 0, 256, 0, 0, 0]
                c32, c64 = vfo.counts32(z, mask, depth, vo.PLATE_K4, DELTA), vfo.counts64(z, mask, depth, vo.PLATE_K4, DELTA)
                assert c32.tolist() == want == c64.tolist(), (t, rect, off, c32, c64)
            rgb = [256, inter, 0, 0, 0, 0, 256, inter]
            assert vfo.counts32(z, mask, None, vo.PLATE_K4, DELTA).tolist() == rgb == vfo.counts64(z, mask, None, vo.PLATE_K4, DELTA).tolist()
    assert [_overlap(PLATES[0][1], r) for r in MASKS] == [64, 256, 36, 0] and [_overlap(PLATES[1][1], r) for r in MASKS] == [0, 256, 56, 0]


def test_plate_with_an_occluder_missing_depth_and_a_see_through_band():
    """Columns 33 .. 40 of the plate 40 mm behind the test depth (front), columns 41 .. 44 missing (0 and NaN), columns 45 .. 46 agreeing,
    47 .. 48 seen through: render 256, valid 192, agree 32, front 128, behind 32, vis 128; the mask holds columns 30 .. 46, rows 23 .. 30."""
    z = _plate_render(PLATES[0][0])
    depth = np.full((PH, PW), 460.0, dtype=F)
    depth[:, 41:43], depth[:, 43:45], depth[:, 45:47], depth[:, 47:] = 0.0, np.nan, 505.0, 540.0
    mask = _rect(30, 46, 23, 30)
    want = [256, 14 * 8, 192, 32, 128, 32, 128, 6 * 8]
    assert vfo.counts32(z, mask, depth, vo.PLATE_K4, DELTA).tolist() == want == vfo.counts64(z, mask, depth, vo.PLATE_K4, DELTA).tolist()
    area = int(mask.sum())
    iou, viou, agree, score = vfo.scores([want], [area], True)
    assert area == 17 * 8 and iou[0] == 112 / (256 + 136 - 112) and viou[0] == 48 / (128 + 136 - 48) and agree[0] == 0.5
    assert score[0] == viou[0] * agree[0] and vfo.scores([want], [area], False)[3][0] == iou[0]


def test_rle_decoder_is_column_major_and_round_trips():
    m = np.zeros((5, 7), dtype=bool)
    m[1:3, 0], m[4, 6] = True, True
    seg = vfo.rle(m)
    assert seg == {"size": [5, 7], "counts": [1, 2, 31, 1]} and np.array_equal(vfo.decode(seg), m)
    rng = np.random.default_rng(2)
    for hw in ((45, 70), (3, 4)):
        r = rng.uniform(size=hw) < 0.5
        assert np.array_equal(vfo.decode(vfo.rle(r)), r)
    assert vfo.rle(np.ones((2, 3), dtype=bool))["counts"] == [0, 6] and vfo.rle(np.zeros((2, 3), dtype=bool))["counts"] == [6]
    from picopose_amd.provider import test_batch as tb
    assert tb.rle_counts(seg).tolist() == [1, 2, 31, 1]


def test_score_formulas_and_their_zero_denominators():
    counts = np.array([[0, 0, 0, 0, 0, 0, 0, 0],          # nothing rendered, an empty mask: every denominator is zero
                       [0, 0, 0, 0, 0, 0, 0, 0],          # nothing rendered, a mask of 50
                       [100, 40, 0, 0, 0, 0, 100, 40],    # RGB only
                       [100, 40, 100, 0, 100, 0, 0, 0],   # all occluded: vis = 0, A > 0
                       [100, 40, 80, 60, 0, 20, 100, 40],
                       [100, 0, 0, 0, 0, 0, 100, 0]])     # rendered, the mask empty
    area = np.array([0, 50, 60, 60, 60, 0])
    for with_depth in (True, False):
        for got in (vfo.scores(counts, area, with_depth), [np.asarray(a) for a in vf.scores(counts, area, with_depth)],
                    [a.numpy() for a in vf.scores(torch.from_numpy(counts.astype(np.int32)), torch.from_numpy(area.astype(np.int32)), with_depth)]):
            iou, viou, agree, score = got
            assert all(a.dtype == np.float64 for a in got)
            assert iou.tolist() == [0.0, 0.0, 40 / 120, 40 / 120, 40 / 120, 0.0]
            assert viou.tolist() == [0.0, 0.0, 40 / 120, 0.0, 40 / 120, 0.0]
            assert agree.tolist() == [1.0, 1.0, 1.0, 1.0, 0.75, 1.0]
            assert score.tolist() == ([0.0, 0.0, 40 / 120, 0.0, (40 / 120) * 0.75, 0.0] if with_depth else iou.tolist())
    assert vf.COUNTS == vfo.NAMES


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_pose_verify_abi_argument_validation_needs_no_gpu():
    from picopose_amd import _lib

    L = _lib.lib()
    assert "pp_pose_verify" in _lib.declared_symbols()
    buf, p = st.aligned_buffer()
    i32, f32, i64 = st.i32, st.f32, st.i64
    H, W = 48, 64
    front = 256 + 1792 + 5 * 8                                     # pp_vsd_workspace_bytes of 200 window samples, 2 + 2 + 1 faces
    need = ctypes.c_size_t()
    assert L.pp_vsd_workspace_bytes(st.WINDOW_SAMPLES, st.VIEW_FACES, ctypes.byref(need)) == 0 and need.value == front
    scene = dict(st.fields(p, H, W), diameters=None)               # the device table `diameters` is not read: null
    own = dict(mask_bits=p, n_masks=2, words=H * W // 32, view_mask=p, view_mask_host=i32(0, 1, 1), depth=p, delta=15.0, workspace=p,
               workspace_bytes=front - 1, counts=p, near_count=p)  # (one byte short: a call that passes every check is PP_EWORKSPACE)
    call = st.caller(L.pp_pose_verify, scene, own)

    assert call() == -2 and call(depth=None) == -2                 # well-formed up to the workspace, with and without depth
    assert call(scene=None) == -1
    for k in [k for k in st.DEVICE_TABLES if k != "diameters"] + list(st.HOST_TABLES) + \
            ["mask_bits", "view_mask", "view_mask_host", "workspace", "counts", "near_count"]:
        assert call(**{k: None}) == -1, k
    for kw in ({"n_objects": 0}, {"n_images": 0}, {"n_views": 0}, {"H": 0}, {"W": -3}, {"near": 0.0}, {"near": float("nan")},
               {"cams_host": f32(100, 100, 32, 24, 90, float("nan"), 30, 20)}, {"cams_host": f32(0, 100, 32, 24, 90, 95, 30, 20)},
               {"diameters_host": f32(100.0, 0.0)}, {"vert_off_host": i32(1, 4, 7)}, {"face_off_host": i32(0, 3, 3)},
               {"faces_host": i32(0, 1, 2, 0, 2, 4, 0, 1, 2)}, {"view_obj_host": i32(0, 2, 1)}, {"view_img_host": i32(0, -1, 1)},
               {"windows_host": i32(0, 0, 10, 10, 55, 38, 65, 48, 5, 5, 5, 9)}, {"view_zoff_host": i64(0, 100, 200, 201)},
               {"n_masks": 0}, {"n_masks": -1}, {"words": H * W // 32 - 1}, {"words": H * W // 32 + 1}, {"words": 0},
               {"H": 47, "windows_host": i32(0, 0, 10, 10, 54, 37, 64, 47, 5, 5, 5, 9)},      # ceil(47 * 64 / 32) = 94 words, not 96
               {"view_mask_host": i32(0, 2, 1)}, {"view_mask_host": i32(0, 1, -1)}, {"n_masks": 1},
               {"delta": -1.0}, {"delta": float("inf")}, {"delta": float("nan")}):
        assert call(**kw) == -1, kw
    assert call(H=47, windows_host=i32(0, 0, 10, 10, 54, 37, 64, 47, 5, 5, 5, 9), words=94) == -2       # (the words follow the frame)
    assert call(workspace=p + 64, workspace_bytes=front) == -2 and call(workspace_bytes=0) == -2
    assert call(delta=0.0) == -2 and call(n_masks=5, view_mask_host=i32(4, 0, 2)) == -2


# ---- host side ------------------------------------------------------------------------------------------------------------------------
def _cpu_models(faces=True):
    objs = vo.objects()
    if not faces:
        del objs[2]["faces"]
    return ev.ObjectModels(objs, device="cpu")


def _seg(hw=(vo.H, vo.W)):
    return vfo.rle(_rect(10, 30, 5, 25, hw))


def test_every_value_error_of_verify_poses_precedes_device_work():
    from picopose_amd import _lib

    m = _cpu_models()
    R, t = np.tile(np.eye(3, dtype=F), (2, 1, 1)), np.tile(F([0, 0, 500]), (2, 1))
    K = np.array([[100.0, 0, 60], [0, 100.0, 45], [0, 0, 1]])
    d = np.zeros((1, vo.H, vo.W), dtype=np.uint16)
    ok = dict(models=m, obj_ids=[1, 2], R=R, t=t, K=K, segmentations=[_seg(), _seg()], size=(vo.H, vo.W), depth=d, depth_scale=1.0)
    bad = [{"obj_ids": [1, 4]}, {"models": _cpu_models(faces=False)}, {"models": None}, {"R": R[:1]}, {"t": t.astype(np.int64)},
           {"K": np.zeros((3, 3))}, {"segmentations": [_seg()]}, {"segmentations": [_seg()] * 3}, {"segmentations": []},
           {"segmentations": [_seg(), _seg((vo.H + 1, vo.W))]}, {"segmentations": [_seg(), {"size": [vo.H, vo.W], "counts": [5]}]},
           {"segmentations": [_seg(), {"counts": [vo.H * vo.W]}]}, {"size": (vo.W, vo.H)}, {"size": 7}, {"size": (0, 5)},
           {"mask_index": [0, 2]}, {"mask_index": [0, -1]}, {"mask_index": [0]}, {"mask_index": [0.0, 1.0]},
           {"segmentations": [_seg()], "mask_index": [0, 1]}, {"depth": d[0]}, {"depth": np.zeros((1, vo.H, vo.W + 1), dtype=F)},
           {"depth_scale": None}, {"depth": None}, {"depth": d.astype(F)}, {"image_index": [0, 1]}, {"image_index": [0]},
           {"delta": -1.0}, {"delta": float("nan")}, {"delta": float("inf")}, {"delta": "15"}, {"delta": True}, {"near": 0.0},
           {"window": "tight"}, {"workspace_bytes": 0}]
    for kw in bad:
        with pytest.raises(ValueError):
            vf.verify_poses(**dict(ok, **kw))
        print("ValueError:", {k: v for k, v in kw.items() if k not in ("models", "segmentations", "depth")} or sorted(kw))
    # well-formed calls reach the device check, and only then fail: CPU models cannot run
    for kw in ({}, {"depth": None, "depth_scale": None}, {"segmentations": [_seg()], "mask_index": [0, 0]}):
        with pytest.raises(_lib.PicoPoseHipError, match="GPU only"):
            vf.verify_poses(**dict(ok, **kw))
    # P = 0: empty tensors, the areas from the runs, no launch (the models are on the CPU)
    e = vf.verify_poses(m, np.zeros(0, dtype=np.int64), R[:0], t[:0], K, [_seg(), _seg()], (vo.H, vo.W), mask_index=np.zeros(0, dtype=np.int64))
    assert tuple(e["counts"].shape) == (0, 8) and e["counts"].dtype == torch.int32 and e["mask_area"].tolist() == [441, 441]
    assert all(tuple(e[k].shape) == (0,) and e[k].dtype == torch.float64 for k in ("iou", "visible_iou", "agreement", "score"))
    assert e["n_groups"] == 0 == e["near_count"]
    e = vf.verify_poses(m, [], R[:0], t[:0], K, [], (vo.H, vo.W))
    assert tuple(e["mask_area"].shape) == (0,) and tuple(e["score"].shape) == (0,)


def _hyp(score, tz):
    return {"inliers_ratio": score, "R_stage_3": np.eye(3, dtype=F).ravel(), "t_stage_3": F([0, 0, tz])}


def _preds():
    return [[_hyp(0.9, 500), _hyp(0.8, 510), _hyp(0.7, 520)], [_hyp(0.6, 600), _hyp(0.5, 610)]]


def test_every_value_error_of_verify_predictions_precedes_device_work(monkeypatch):
    def never(*a, **kw):
        raise AssertionError("verify_poses must not be reached")
    monkeypatch.setattr(vf, "verify_poses", never)
    m = _cpu_models()
    K = np.array([[100.0, 0, 60], [0, 100.0, 45], [0, 0, 1]])
    ok = dict(preds_image=_preds(), models=m, obj_ids=[1, 2], K=K, segmentations=[_seg(), _seg()], size=(vo.H, vo.W))
    no_key = _preds()
    del no_key[1][1]["R_stage_3"]
    bad = [{"stage": "stage_2"}, {"stage": None}, {"stage": "depth"}, {"stage": "rgbd"}, {"hypotheses": "first"}, {"hypotheses": "best"},
           {"rank": 1}, {"obj_ids": [1]}, {"segmentations": [_seg()]}, {"depth": np.zeros((2, vo.H, vo.W), dtype=F)},
           {"depth": np.zeros(5, dtype=F)}, {"preds_image": no_key}]
    for kw in bad:
        with pytest.raises(ValueError):
            pl.verify_predictions(**dict(ok, **kw))
    monkeypatch.undo()
    with pytest.raises(ValueError, match="delta"):              # verify_poses' own, still before the device
        pl.verify_predictions(**dict(ok, delta=-1.0))
    with pytest.raises(ValueError, match="size"):
        pl.verify_predictions(**dict(ok, segmentations=[_seg(), _seg((vo.H + 1, vo.W))]))


def test_rank_orders_by_score_keeps_ties_and_leaves_the_input_alone(monkeypatch):
    seen = {}

    def fake(models, obj_ids, R, t, K, segmentations, size, mask_index=None, depth=None, depth_scale=None, **kw):
        seen.update(obj_ids=list(obj_ids), mask_index=list(mask_index), tz=[float(v[2]) for v in t], depth=depth, kw=kw, n_seg=len(segmentations))
        score = torch.tensor(seen["scores"][:len(obj_ids)], dtype=torch.float64)
        counts = torch.arange(8 * len(obj_ids), dtype=torch.int32).reshape(-1, 8)
        return {"counts": counts, "mask_area": torch.zeros(2, dtype=torch.int32), "iou": score / 2, "visible_iou": score / 4, "agreement": score / 8,
                "score": score, "near_count": 0, "n_groups": 1}
    monkeypatch.setattr(vf, "verify_poses", fake)
    m, K = object(), np.eye(3)
    preds = _preds()
    seen["scores"] = [0.25, 0.5, 0.25, 0.75, 0.75]
    out = pl.verify_predictions(preds, m, [1, 2], K, [_seg(), _seg()], (vo.H, vo.W), delta=10.0)
    assert seen["obj_ids"] == [1, 1, 1, 2, 2] and seen["mask_index"] == [0, 0, 0, 1, 1] and seen["tz"] == [500.0, 510.0, 520.0, 600.0, 610.0]
    assert seen["depth"] is None and seen["kw"] == {"delta": 10.0} and seen["n_seg"] == 2
    # instance 0: the best score first, then the tie in its inlier-ratio order; instance 1: a full tie keeps the order
    assert [h["inliers_ratio"] for h in out[0]] == [0.8, 0.9, 0.7] and [h["inliers_ratio"] for h in out[1]] == [0.6, 0.5]
    assert [h["verify_score"] for h in out[0]] == [0.5, 0.25, 0.25]
    first = out[0][0]
    assert set(pl.VERIFY_KEYS) <= set(first) and first["verify_iou"] == 0.25 and first["verify_visible_iou"] == 0.125 and first["verify_agreement"] == 0.0625
    assert first["verify_counts"] == list(range(8, 16)) and all(type(c) is int for c in first["verify_counts"]) and type(first["verify_score"]) is float
    assert all("verify_score" not in h for hyps in preds for h in hyps) and [h["inliers_ratio"] for h in preds[0]] == [0.9, 0.8, 0.7]
    lines = pl.bop_csv_lines(3, 7, [1, 2], [0.5, 0.4], out, 0.1)
    assert lines[0].split(",")[5] == "0.0 0.0 510.0" and lines[1].split(",")[5] == "0.0 0.0 600.0"
    # rank=False keeps the order; "best" verifies the first hypothesis of each instance only
    kept = pl.verify_predictions(preds, m, [1, 2], K, [_seg(), _seg()], (vo.H, vo.W), rank=False)
    assert [h["inliers_ratio"] for h in kept[0]] == [0.9, 0.8, 0.7] and kept[0][1]["verify_score"] == 0.5
    best = pl.verify_predictions(preds, m, [1, 2], K, [_seg(), _seg()], (vo.H, vo.W), hypotheses="best", rank=False,
                                 depth=np.zeros((vo.H, vo.W), dtype=F))
    assert seen["mask_index"] == [0, 1] and tuple(seen["depth"].shape) == (1, vo.H, vo.W)
    assert "verify_score" in best[0][0] and "verify_score" not in best[0][1] and "verify_score" in best[1][0]
    assert pl.verify_predictions([], m, [], K, [], (vo.H, vo.W)) == []
