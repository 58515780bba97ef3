"""CPU: the VSD oracle (tests/vsd_oracle.py) against closed-form answers that do not come from it, the host side of
picopose_amd/evaluation.py's VSD path — the window planner, score_errors(vsd=...), match_and_score's image requests, every ValueError —
and the argument checks of pp_vsd_errors / pp_vsd_workspace_bytes through the ABI (no GPU)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_oracle as ro  # noqa: E402
import scene_tables as st  # noqa: E402
import vsd_oracle as vo  # noqa: E402

from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import scene as scn  # noqa: E402
from picopose_amd.evaluation import vsd_errors  # noqa: E402,F401  (absent before the feature: every test here fails without it)

F = np.float32


def _plate_pair(est, gt, test):
    p = vo.plate(vo.PLATE_N)
    H, W = vo.PLATE_HW
    z = [vo.depth32(p["vertices"], p["faces"], P, vo.PLATE_K4, H, W)[0] for P in (est, gt)]
    return z, vo.vsd32(z[0], z[1], test, vo.PLATE_K4, vo.PLATE_DIAMETER), vo.vsd64(z[0], z[1], test, vo.PLATE_K4, vo.PLATE_DIAMETER)


@pytest.mark.parametrize("name", sorted(vo.plate_cases()))
def test_oracle_closed_forms_on_the_plate(name):
    """The fronto-parallel n x n-sample plate (f = 100, Z = 500 mm, side 5 n mm, principal point at half-integers, n = 16):
    identical poses: e = 0; a shift of k columns with the test depth missing: union n (n + k), inter n (n - k), e = 2 k / (n + k) at every
    tau; an occluder 200 mm in front of the left half halves the union and keeps e = 0; a surface behind the plate changes nothing; an
    estimate 30 mm behind a VISIBLE ground truth is visible through the visib_gt clause, and dd = 30 r / diameter lies in 0.2651 .. 0.2667
    (1 <= r <= 1.0057), above tau = 0.25 and below 0.30 by more than 1 %: e = 1 up to 0.25, 0 from 0.30; the same with the depth missing;
    two plates off the frame: union 0, e = 1.  The float32 and the float64 statements agree on all of them."""
    est, gt, test, want = vo.plate_cases()[name]
    z, (c32, e32), (c64, e64) = _plate_pair(est, gt, test)
    assert c32[0] == want["union"] and c32[1] == want["inter"], (name, c32)
    assert np.array_equal(c32, c64)
    assert np.allclose(e64, want["e"], rtol=0, atol=1e-15) and np.array_equal(e32, want["e"].astype(F)), (name, e32, want["e"])
    if name == "identical":
        assert (z[0] > 0).sum() == vo.PLATE_N ** 2 and np.abs(z[0][z[0] > 0].astype(np.float64) - 500.0).max() <= 8 * vo.U32 * 500.0
    if name in ("gt_clause", "offset"):
        r = vo._rays32(vo.PLATE_K4, *vo.PLATE_HW)[z[1] > 0].astype(np.float64)
        dd = 30.0 * r / vo.PLATE_DIAMETER
        assert dd.min() > 0.25 * 1.01 and dd.max() < 0.30 / 1.01


def test_depth32_window_equals_the_full_frame_inside_it():
    m = ro.icosphere(2, 50.0)
    P = vo.pose(vo.random_rotation(np.random.default_rng(0)), (20.0, -10.0, 450.0))
    z, _ = vo.depth32(m["vertices"], m["faces"], P, vo.CAMS[0], vo.H, vo.W)
    win = (60, 30, 75, 52)
    zw, _ = vo.depth32(m["vertices"], m["faces"], P, vo.CAMS[0], vo.H, vo.W, window=win)
    inside = np.zeros_like(z, dtype=bool)
    inside[win[1]:win[3], win[0]:win[2]] = True
    assert (z > 0).sum() > 300 and np.array_equal(zw[inside].view(np.int32), z[inside].view(np.int32)) and np.all(zw[~inside] == 0)
    assert vo.depth32(m["vertices"], m["faces"], P, vo.CAMS[0], vo.H, vo.W, window=(5, 5, 5, 9))[0].max() == 0


def test_window_planner_contains_the_full_frame_coverage():
    """Random poses, partly and wholly off the frame among them: the planned window holds every covered sample of the full-frame
    render (so the windowed render has the same bits); a pose that straddles the near plane falls back to the whole frame; an
    off-frame object and a non-finite pose get the empty window."""
    rng = np.random.default_rng(5)
    meshes = [ro.cube(40.0), ro.icosphere(2, 50.0)]
    seen = {"inside": 0, "partly": 0, "off": 0}
    for k in range(60):
        m = meshes[k % 2]
        corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * np.abs(m["vertices"]).max(axis=0)
        P = vo.pose(vo.random_rotation(rng), (rng.uniform(-400, 400), rng.uniform(-300, 300), rng.uniform(250, 700)))
        cam = vo.CAMS[k % 2]
        win = ev.plan_window(corners, P, cam.astype(np.float64), vo.H, vo.W, 1.0)
        z, _ = vo.depth32(m["vertices"], m["faces"], P, cam, vo.H, vo.W)
        ys, xs = np.where(z > 0)
        assert 0 <= win[0] <= win[2] <= vo.W and 0 <= win[1] <= win[3] <= vo.H
        if len(xs):
            assert win[0] <= xs.min() and xs.max() < win[2] and win[1] <= ys.min() and ys.max() < win[3], (k, win)
            full = xs.min() > 0 and ys.min() > 0 and xs.max() < vo.W - 1 and ys.max() < vo.H - 1
            seen["inside" if full else "partly"] += 1
            assert (win[2] - win[0]) * (win[3] - win[1]) < vo.H * vo.W
        else:
            seen["off"] += 1
    assert min(seen.values()) >= 3, seen
    corners = np.array([[x, y, z] for x in (-40, 40) for y in (-40, 40) for z in (-40, 40)], dtype=np.float64)
    assert ev.plan_window(corners, vo.pose(t=(0, 0, 30.0)), (100, 100, 60, 45), vo.H, vo.W, 1.0) == (0, 0, vo.W, vo.H)      # straddles near
    assert ev.plan_window(corners, vo.pose(t=(0, 0, 41.5)), (100, 100, 60, 45), vo.H, vo.W, 1.0) != (0, 0, 0, 0)
    assert ev.plan_window(corners, vo.pose(t=(9000.0, 0, 500.0)), (100, 100, 60, 45), vo.H, vo.W, 1.0) == (0, 0, 0, 0)
    bad = vo.pose()
    bad[1, 3] = np.nan
    assert ev.plan_window(corners, bad, (100, 100, 60, 45), vo.H, vo.W, 1.0) == (0, 0, 0, 0)


class _Models:
    """What score_errors needs of an ObjectModels."""

    def __init__(self, diam):
        self._d = diam

    def diameter(self, o):
        return self._d[int(o)]


def _protocol_inputs(rng, n_images=6):
    targets, pairs, scores = [], {"target": [], "est": [], "gt": []}, []
    for im in range(n_images):
        for obj in (1, 2):
            count = 1 + (im + obj) % 2
            targets.append((1, im, obj, count))
            ests = list(range(len(scores), len(scores) + count))
            scores += rng.uniform(0.1, 1.0, count).tolist()
            for e in ests:
                for g in range(count):
                    pairs["target"].append(len(targets) - 1)
                    pairs["est"].append(e)
                    pairs["gt"].append(g)
    return np.array(targets), {k: np.array(v, dtype=np.int64) for k, v in pairs.items()}, np.array(scores)


def test_score_errors_vsd_recalls_equal_a_brute_force_restatement():
    rng = np.random.default_rng(2)
    targets, pairs, scores = _protocol_inputs(rng)
    n = len(pairs["est"])
    e = rng.choice([0.0, 0.04, 0.12, 0.27, 0.33, 0.51, 1.0], size=(n, 10)).astype(F)
    e.sort(axis=1)
    e = e[:, ::-1].copy()                                         # e_tau falls as tau grows
    big = np.full(n, 1e9)
    res = ev.score_errors(pairs, big, big, scores, targets, _Models({1: 100.0, 2: 80.0}),
                          vsd={"errors": e, "taus": ev.VSD_TAUS, "thresholds": ev.VSD_THRESHOLDS, "delta": 15.0})
    want = np.zeros((10, 10))
    for k in range(10):
        for j, th in enumerate(ev.VSD_THRESHOLDS):
            for t in range(len(targets)):
                rows = np.where(pairs["target"] == t)[0]
                used = set()
                for est in sorted(set(pairs["est"][rows].tolist()), key=lambda i: (-scores[i], i)):
                    cand = [(float(e[i, k]), int(pairs["gt"][i])) for i in rows if pairs["est"][i] == est and pairs["gt"][i] not in used
                            and float(e[i, k]) < th]
                    if cand:
                        used.add(min(cand)[1])
                        want[k, j] += 1
    want /= targets[:, 3].sum()
    assert res["recall_vsd"].shape == (10, 10) and np.array_equal(res["recall_vsd"], want) and len(np.unique(want)) > 5
    assert res["AR_VSD"] == want.mean() and res["AR_MSSD"] == 0 and res["AR"] == want.mean() / 3
    assert set(res["per_object"][1]) >= {"recall_vsd", "AR_VSD", "AR"} and res["vsd"]["delta"] == 15.0
    plain = ev.score_errors(pairs, big, big, scores, targets, _Models({1: 100.0, 2: 80.0}))
    assert plain["vsd"] is None and "AR" not in plain and "recall_vsd" not in plain and "AR_VSD" not in plain["per_object"][1]


def test_match_and_score_requests_only_the_images_of_pairs(monkeypatch):
    """pose_errors and vsd_errors are replaced by recorders (no GPU): without depth_images the result is today's; a callable and a dict
    are asked for the same images — those with pairs — images_per_call at a time, with the cameras' scales."""
    import torch

    rng = np.random.default_rng(4)
    n_im = 5
    gt = {1: {im: {"obj_id": np.array([7]), "R": np.eye(3)[None], "t": np.array([[0.0, 0, 500.0 + im]])} for im in range(n_im)}}
    cams = {1: {im: {"K": np.array([[100.0, 0, 60], [0, 100.0, 45], [0, 0, 1]]), "depth_scale": 0.1 * (im + 1)} for im in range(n_im + 1)}}
    est = {"scene_id": np.ones(4, dtype=np.int64), "im_id": np.array([0, 2, 3, 9]), "obj_id": np.full(4, 7), "score": rng.uniform(size=4),
           "R": np.tile(np.eye(3), (4, 1, 1)), "t": np.tile([0.0, 0, 510.0], (4, 1))}
    targets = np.array([[1, im, 7, 1] for im in range(n_im)] + [[1, 9, 7, 1]])
    calls = []

    def fake_pose_errors(models, obj, *a, **kw):
        return {"mssd": torch.zeros(len(obj)), "mspd": torch.zeros(len(obj))}

    def fake_vsd_errors(models, obj, Re, te, Rg, tg, K, depth, image_index=None, depth_scale=None, delta=15.0, taus=None, **kw):
        calls.append({"n": len(obj), "shape": depth.shape, "dtype": depth.dtype, "scale": None if depth_scale is None else list(depth_scale),
                      "index": image_index.tolist(), "K": np.asarray(K).shape, "delta": delta})
        return {"vsd": torch.full((len(obj), len(taus)), 0.2)}

    monkeypatch.setattr(ev, "pose_errors", fake_pose_errors)
    monkeypatch.setattr(ev, "vsd_errors", fake_vsd_errors)
    models = _Models({7: 100.0})
    base = ev.match_and_score(est, gt, targets, models, cams)
    assert base["vsd"] is None and "AR" not in base and not calls and base["AR_MSSD"] == 3 / 6
    asked = []
    frames = {1: {im: np.full((9, 12), im, dtype=np.uint16) for im in range(n_im)}}

    def loader(scene, im):
        asked.append((scene, im))
        return frames[scene][im]

    a = ev.match_and_score(est, gt, targets, models, cams, depth_images=loader, images_per_call=2, vsd_delta=12.0)
    by_call, calls[:] = list(calls), []
    b = ev.match_and_score(est, gt, targets, models, cams, depth_images=frames, images_per_call=2, vsd_delta=12.0)
    assert asked == [(1, 0), (1, 2), (1, 3)] and by_call == calls and [c["n"] for c in calls] == [2, 1]
    assert calls[0]["shape"] == (2, 9, 12) and calls[0]["dtype"] == np.uint16 and np.allclose(calls[0]["scale"], [0.1, 0.3])
    assert calls[0]["index"] == [0, 1] and calls[0]["K"] == (2, 3, 3) and calls[0]["delta"] == 12.0
    for r in (a, b):
        assert r["vsd"]["errors"].shape == (3, 10) and np.all(r["vsd"]["errors"] == F(0.2))
        assert np.array_equal(r["recall_vsd"][0], (0.2 < ev.VSD_THRESHOLDS) * 0.5) and r["AR"] == (r["AR_VSD"] + r["AR_MSSD"] + r["AR_MSPD"]) / 3
        assert {k: v for k, v in r.items() if k in ("AR_MSSD", "AR_MSPD", "n_targets")} == {k: base[k] for k in ("AR_MSSD", "AR_MSPD", "n_targets")}
    with pytest.raises(ValueError, match="resolution"):
        ev.match_and_score(est, gt, targets, models, cams, depth_images={1: {**frames[1], 2: np.zeros((9, 13), dtype=np.uint16)}})


def _cpu_models(faces=True):
    objs = vo.objects()
    if not faces:
        del objs[2]["faces"]
    return ev.ObjectModels(objs, device="cpu")


def test_object_models_take_faces_and_keep_working_without():
    m = _cpu_models()
    assert m.has_faces and [m.n_faces(o) for o in (1, 2, 3)] == [12, 1280, 2] and m.face_off.tolist() == [0, 12, 1292, 1294]
    assert m.faces_host.dtype == np.int32 and m.faces_host.max() == 641 and tuple(m.faces.shape) == (1294, 3)
    part = _cpu_models(faces=False)
    assert not part.has_faces and part.n_faces(2) == 0 and part.n_faces(1) == 12
    none = ev.ObjectModels({1: {"vertices": ro.cube(40.0)["vertices"], "info": {"diameter": 100.0}}}, device="cpu")
    assert not none.has_faces and none.faces is None
    v = ro.cube(40.0)["vertices"]
    for f in (np.zeros((0, 3), dtype=np.int32), np.zeros((4, 2), dtype=np.int32), np.zeros((4, 3)), np.array([[0, 1, 8]]), np.array([[0, -1, 2]])):
        with pytest.raises(ValueError, match="face"):
            ev.ObjectModels({1: {"vertices": v, "faces": f, "info": {"diameter": 100.0}}}, device="cpu")


def test_every_value_error_of_the_vsd_entry_points():
    m = _cpu_models()
    R, t = np.tile(np.eye(3, dtype=F), (2, 1, 1)), np.tile(F([0, 0, 500]), (2, 1))
    K = np.array([[100.0, 0, 60], [0, 100.0, 45], [0, 0, 1]])
    d = np.zeros((2, vo.H, vo.W), dtype=np.uint16)
    ok = dict(models=m, obj_ids=[1, 2], R_est=R, t_est=t, R_gt=R, t_gt=t, K=K, depth=d, depth_scale=1.0)
    bad = [{"obj_ids": [1, 4]}, {"obj_ids": [1.0, 2.0]}, {"models": _cpu_models(faces=False)}, {"models": None}, {"R_est": R[:1]},
           {"t_gt": t.astype(np.int64)}, {"K": K[:2]}, {"K": np.zeros((3, 3, 3))}, {"K": np.zeros((3, 3))}, {"depth": d[0]},
           {"depth": d.astype(np.int32)}, {"depth_scale": None}, {"depth_scale": -1.0}, {"depth": d.astype(F)}, {"depth": [[0]]},
           {"image_index": [0, 2]}, {"image_index": [0]}, {"image_index": [0.0, 1.0]}, {"taus": []}, {"taus": np.arange(17) / 20.0},
           {"taus": [[0.1]]}, {"taus": [np.nan]}, {"delta": 0.0}, {"near": -1.0}, {"window": "tight"}, {"workspace_bytes": 0}]
    for kw in bad:
        with pytest.raises(ValueError):
            ev.vsd_errors(**dict(ok, **kw))
        print("ValueError:", kw if "models" not in kw else "models")
    with pytest.raises(ValueError, match="vsd"):
        ev.pose_errors(m, [1], R[:1], t[:1], R[:1], t[:1], K=K, kinds=("mssd", "vsd"))
    empty = ev.vsd_errors(m, np.zeros(0, dtype=np.int64), R[:0], t[:0], R[:0], t[:0], K, d, depth_scale=1.0, taus=[0.1, 0.2])
    assert tuple(empty["vsd"].shape) == (0, 2) and tuple(empty["n_far"].shape) == (0, 2) and empty["n_views"] == 0 and empty["near_count"] == 0
    for kw in ({"resolution": (0, 5)}, {"resolution": 7}, {"obj_ids": [1, 9]}, {"window": None}, {"image_index": [0, 1]}, {"R": R[:1]}):
        with pytest.raises(ValueError):
            ev.render_depth(**dict(dict(models=m, obj_ids=[1, 2], R=R, t=t, K=K, resolution=(vo.H, vo.W)), **kw))
    none = ev.render_depth(m, [], R[:0], t[:0], K, (vo.H, vo.W))
    assert tuple(none["depth"].shape) == (0, vo.H, vo.W) and none["near_count"] == 0


def test_view_groups_split_the_pairs_under_the_workspace_bound():
    m = _cpu_models()
    view_obj = np.array([0, 0, 1, 1, 1], dtype=np.int32)
    windows = np.array([[0, 0, 10, 10]] * 5, dtype=np.int32)
    pe, pg = np.array([0, 2, 3], dtype=np.int32), np.array([1, 4, 4], dtype=np.int32)
    one = scn.view_groups(m, view_obj, windows, pe, pg, 1 << 30)
    assert len(one) == 1 and one[0][0].tolist() == [0, 1, 2, 4, 3] and one[0][1].tolist() == [0, 1, 2]
    tiny = scn.view_groups(m, view_obj, windows, pe, pg, 1)
    assert [g[0].tolist() for g in tiny] == [[0, 1], [2, 4], [3, 4]] and [g[1].tolist() for g in tiny] == [[0], [1], [2]]
    assert [g[0].tolist() for g in scn.view_groups(m, view_obj, windows, None, None, 1)] == [[0], [1], [2], [3], [4]]


def test_vsd_abi_argument_validation_needs_no_gpu():
    from picopose_amd import _lib

    L = _lib.lib()
    assert {"pp_vsd_errors", "pp_vsd_workspace_bytes"} <= set(_lib.declared_symbols())
    need = ctypes.c_size_t()
    assert L.pp_vsd_workspace_bytes(1000, 24, ctypes.byref(need)) == 0 and need.value == 256 + 8192 + 24 * 8
    assert L.pp_vsd_workspace_bytes(0, 24, ctypes.byref(need)) == 0 and need.value == 256 + 24 * 8
    for args in ((-1, 24), (10, 0), (10, 2 ** 32), (2 ** 62, 1)):
        assert L.pp_vsd_workspace_bytes(*args, ctypes.byref(need)) == -1, args
    assert L.pp_vsd_workspace_bytes(10, 10, None) == -1
    buf, p = st.aligned_buffer()
    i32, f32, i64 = st.i32, st.f32, st.i64
    scene = st.fields(p)
    ws_bytes = 256 + 8 * st.WINDOW_SAMPLES + 192 + 8 * st.VIEW_FACES          # 1600 z-buffer bytes rounded up to 1792
    own = dict(pair_est=p, pair_gt=p, pair_est_host=i32(0, 2), pair_gt_host=i32(1, 2), n_pairs=2, depth=p, delta=15.0, taus_host=f32(0.1, 0.2),
               n_taus=2, workspace=p, workspace_bytes=ws_bytes, vsd=p, counts=p, near_count=p, depth_out=None)
    call = st.caller(L.pp_vsd_errors, scene, own)

    # (a valid argument list would launch: it is never sent here; every call below differs from it in one invalid argument)
    assert call(scene=None) == -1
    for k in st.DEVICE_TABLES + st.HOST_TABLES + tuple(k for k, v in own.items() if v is p or isinstance(v, ctypes.Array)):
        assert call(**{k: None}) == -1, k
    for kw in ({"n_objects": 0}, {"n_images": 0}, {"n_views": 0}, {"n_pairs": -1}, {"n_pairs": 0}, {"H": 0}, {"W": -3}, {"H": 50000, "W": 50000},
               {"n_taus": 0}, {"n_taus": 17},
               {"delta": 0.0}, {"delta": float("inf")}, {"delta": float("nan")}, {"near": 0.0}, {"near": float("inf")}, {"taus_host": f32(0.1, float("nan"))},
               {"diameters_host": f32(100.0, 0.0)}, {"diameters_host": f32(float("inf"), 50.0)}, {"cams_host": f32(0, 100, 32, 24, 90, 95, 30, 20)},
               {"cams_host": f32(100, 100, 32, 24, 90, float("nan"), 30, 20)}, {"vert_off_host": i32(1, 4, 7)}, {"vert_off_host": i32(0, 4, 4)},
               {"face_off_host": i32(0, 2, 1)}, {"face_off_host": i32(0, 3, 3)},                             # (object 1 of view 2 has no faces)
               {"faces_host": i32(0, 1, 2, 0, 2, 4, 0, 1, 2)}, {"faces_host": i32(0, 1, 2, 0, 2, 3, 0, 1, 3)},
               {"faces_host": i32(0, -1, 2, 0, 2, 3, 0, 1, 2)},
               {"view_obj_host": i32(0, 2, 1)}, {"view_img_host": i32(0, -1, 1)}, {"windows_host": i32(0, 0, 10, 10, 55, 38, 65, 48, 5, 5, 5, 9)},
               {"windows_host": i32(0, 0, 10, 10, 54, 39, 64, 49, 5, 5, 5, 9)}, {"windows_host": i32(-1, 0, 9, 10, 54, 38, 64, 48, 5, 5, 5, 9)},
               {"windows_host": i32(0, 0, 10, 10, 54, 38, 64, 48, 6, 5, 5, 9)}, {"view_zoff_host": i64(0, 100, 200, 201)},
               {"view_zoff_host": i64(1, 101, 201, 201)},
               {"pair_est_host": i32(0, 3)}, {"pair_gt_host": i32(-1, 2)}, {"pair_gt_host": i32(1, 0)},
               {"pair_est_host": i32(2, 2), "pair_gt_host": i32(0, 2)}):
        assert call(**kw) == -1, kw
    # PP_EWORKSPACE.  These calls pass every check of the scene before they fail on the workspace, so they are also the guard that the
    # ctypes layout of _lib.PpScene is the C struct's: a shifted member would fail a scene check with -1 instead.
    assert call(workspace_bytes=ws_bytes - 1) == -2 and call(workspace=p + 64) == -2 and call(workspace_bytes=0) == -2
