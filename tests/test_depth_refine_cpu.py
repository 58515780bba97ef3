"""CPU: the depth refinement's oracle (tests/depth_refine_oracle.py) against closed forms, the properties of the test scenes that the
GPU tests rely on (no fragile sample, few steps near the rank cut, the oracle converges), and everything of picopose_amd/depth_refine.py
and pipeline.refine_predictions that needs no device: argument validation, the window and grouping plan, the ranking, the C entry's
PP_EINVAL paths."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_refine_oracle as do  # noqa: E402
import scene_tables as st  # noqa: E402
import vsd_oracle as vo  # noqa: E402

from picopose_amd import depth_refine as dr  # noqa: E402  (absent before the feature: every test here fails without it)
from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import pipeline  # noqa: E402
from picopose_amd import scene as scn  # noqa: E402

F = np.float32


def _plate():
    p = vo.plate(vo.PLATE_N)
    return {"vertices": p["vertices"], "faces": p["faces"], "info": {"diameter": vo.PLATE_DIAMETER}}


def test_plate_against_a_flat_depth_moves_along_its_normal_with_rank_3():
    """The 16 x 16 plate at Z = 500 facing the camera, test depth 520 everywhere: every one of the 256 samples has n = (0, 0, -1) and
    r = n . (p_t - p_m) = -20, the rows are [(q x n) / rho, n] with q in the plate's plane: J^T J couples only (theta_x, theta_y, v_z), so
    rank 3; the samples are symmetric about the centre (half-integer principal point), so J^T r has only the v_z entry and the step is
    v = (0, 0, 20).  In-plane translation and the rotation about the normal get exactly 0."""
    obj, (H, W) = _plate(), vo.PLATE_HW
    P = vo.pose()
    win = do.plan(obj, P, vo.PLATE_K4, H, W)
    sums, N, fragile = do.linearise(P, obj, vo.PLATE_K4, np.full((H, W), 520.0, dtype=F), win)
    assert N == vo.PLATE_N ** 2 and fragile == 0 and sums[28] == N and abs(sums[27] - 400.0 * N) < 2e-5 * 400 * N   # (Z_r is a float32 render: a few ulps of 500)
    P1, rank, info = do.step(sums, P, obj, full=True)
    assert rank == 3
    x = info["x"]
    assert x[2] == 0 and x[3] == 0 and x[4] == 0 and abs(x[5] - 20.0) < 1e-4 and np.abs(x[:2]).max() < 1e-4
    assert np.array_equal(P1[:2, 3], P[:2, 3]) and abs(float(P1[2, 3]) - 520.0) < 1e-4
    assert np.abs(P1[:3, :3] - np.eye(3)).max() < 1e-6 and abs(P1[0, 1]) < 1e-12 and abs(P1[1, 0]) < 1e-12      # no rotation about the normal
    out = do.run(P, obj, vo.PLATE_K4, np.full((H, W), 520.0, dtype=F), win, **dict(do.DEFAULTS, min_points=100))
    assert out["status"] == 0 and out["iterations"] == 2 and out["rank"] == 3 and out["rms_after"] < 1e-3 and abs(out["rms_before"] - 20) < 1e-3


def test_icosphere_against_its_own_render_recovers_the_translation_with_rank_3():
    """A sphere's rotation is invisible to depth.  The 1280 flat faces of the icosphere make it faintly visible (eigenvalues of about
    1e-3 lambda_max, asserted), so this closed form uses rcond = 0.05: three directions are kept, the pose only translates, and
    it lands on the ground truth's translation.  The three kept eigenvectors are translations up to the facets' small coupling
    with the rotations, so the rotation stays within 1e-3 rad of the input's."""
    obj = vo.objects()[2]
    Pg, Ps = vo.pose(t=(10, -5, 500)), vo.pose(t=(13, -3, 512))
    z, face = do.zbuffer(obj["vertices"], obj["faces"], Pg, vo.CAMS[0], vo.H, vo.W)
    assert (face >= 0).sum() > 250
    depth = np.where(z > 0, z, F(1500))
    win = do.plan(obj, Ps, vo.CAMS[0], vo.H, vo.W)
    sums, N, _ = do.linearise(Ps, obj, vo.CAMS[0], depth, win)
    _, rank, info = do.step(sums, Ps, obj, rcond=0.05, full=True)
    assert rank == 3 and info["eig"][3] > 100 * info["eig"][2] and 1e-5 * info["eig"][5] < info["eig"][0] < 1e-2 * info["eig"][5]
    out = do.run(Ps, obj, vo.CAMS[0], depth, win, **dict(do.DEFAULTS, min_points=50, rcond=0.05))
    assert out["status"] in (0, 1) and out["rank"] == 3
    assert np.abs(out["pose"][:3, 3].astype(np.float64) - [10, -5, 500]).max() < 0.05, out["pose"][:3, 3]
    assert np.abs(out["pose"][:3, :3] - np.eye(3)).max() < 1e-3


def test_zbuffer_keeps_the_winning_face_and_equals_depth32():
    obj = vo.objects()[1]
    P = vo.pose(vo.random_rotation(np.random.default_rng(2)), (20, -10, 450))
    z, face = do.zbuffer(obj["vertices"], obj["faces"], P, vo.CAMS[1], vo.H, vo.W)
    ref, _ = vo.depth32(obj["vertices"], obj["faces"], P, vo.CAMS[1], vo.H, vo.W)
    assert np.array_equal(z.view(np.int32), ref.view(np.int32)) and np.array_equal(face >= 0, ref > 0)
    assert face.max() < 12 and len(np.unique(face[face >= 0])) >= 3


def test_the_scenes_of_the_gpu_tests_are_decidable_and_the_oracle_converges():
    """What tests/test_depth_refine_gpu.py takes for granted: no sample of the mixed scene's first linearisations or of any step of
    the two scenes is fragile, at most 5 % of the steps have an eigenvalue within 10 % of the rank cut, every status the edge tests do
    not cover occurs, and on the convergence scene the oracle's final MSSD is below a tenth of the start's."""
    scene, dm, poses, wins = do.mixed()
    runs = do.mixed_runs() + do.convergence_runs()
    assert all(f == 0 for r in runs for f in r["fragile"])
    steps = [m for r in runs for m in r["cut_margin"]]
    assert len(steps) >= 40 and sum(m < 0.1 for m in steps) <= 0.05 * len(steps)
    assert {r["status"] for r in runs} >= {0, 1, 2, 3}
    assert sum(r["n_points"] for r in do.mixed_runs()) > 2000 and len({r["rank"] for r in runs}) >= 3
    sc = do.convergence_scene()
    for p, r in enumerate(do.convergence_runs()):
        obj = sc["objects"][int(sc["obj_ids"][p])]
        start, final = do.mssd(obj, sc["start"][p], sc["gt"][p]), do.mssd(obj, r["pose"], sc["gt"][p])
        print(f"pose {p}: MSSD {start:.3f} -> {final:.4f} mm, status {r['status']}, {r['iterations']} iterations, rank {r['rank']}")
        assert r["status"] in (0, 1) and start > 19.9 and final < 0.1 * start


def _cpu_models(faces=True):
    objs = vo.objects()
    if not faces:
        del objs[2]["faces"]
    return ev.ObjectModels(objs, device="cpu")


def test_every_value_error_of_refine_poses_depth():
    m = _cpu_models()
    R, t = np.tile(np.eye(3, dtype=F), (2, 1, 1)), np.tile(F([0, 0, 500]), (2, 1))
    K = np.array([[100.0, 0, 60], [0, 100.0, 45], [0, 0, 1]])
    d = np.zeros((2, vo.H, vo.W), dtype=np.uint16)
    ok = dict(models=m, obj_ids=[1, 2], R=R, t=t, K=K, depth=d, depth_scale=1.0)
    bad = [{"obj_ids": [1, 4]}, {"obj_ids": [1.0, 2.0]}, {"models": _cpu_models(faces=False)}, {"models": None}, {"R": R[:1]},
           {"t": t.astype(np.int64)}, {"K": K[:2]}, {"K": np.zeros((3, 3))}, {"depth": d[0]}, {"depth": d.astype(np.int32)},
           {"depth_scale": None}, {"depth_scale": -1.0}, {"depth": d.astype(F)}, {"image_index": [0, 2]}, {"image_index": [0]},
           {"iterations": 0}, {"iterations": 1001}, {"iterations": 2.0}, {"iterations": True}, {"max_distance": 0.0},
           {"max_distance": math.inf}, {"min_points": 0}, {"min_points": 10.5}, {"min_cos": -0.1}, {"min_cos": 1.0}, {"min_cos": math.nan},
           {"rcond": -1e-6}, {"rcond": 1.0}, {"eps": -1.0}, {"eps": math.inf}, {"margin": -1}, {"margin": 1.5}, {"max_translation": 0.0},
           {"max_rotation": 0.0}, {"max_rotation": math.nan}, {"near": 0.0}, {"workspace_bytes": 0}, {"debug": 1}]
    for kw in bad:
        with pytest.raises(ValueError):
            dr.refine_poses_depth(**dict(ok, **kw))
        print("ValueError:", kw if "models" not in kw else "models")
    with pytest.raises(TypeError):
        dr.refine_poses_depth(m, [1, 2], R, t, K, d, None, 1.0, 10)            # the parameters are keyword-only
    empty = dr.refine_poses_depth(m, np.zeros(0, dtype=np.int64), R[:0], t[:0], K, d, depth_scale=1.0, iterations=3, debug=True)
    assert tuple(empty["R"].shape) == (0, 3, 3) and tuple(empty["t"].shape) == (0, 3) and empty["n_groups"] == 0
    assert tuple(empty["trajectory"].shape) == (0, 4, 4, 4) and tuple(empty["sums"].shape) == (0, 3, 29)
    assert all(tuple(empty[k].shape) == (0,) for k in ("status", "iterations", "rank", "n_points", "rms_before", "rms_after", "near_count"))


def test_window_margin_strips_and_grouping_plan():
    m = _cpu_models()
    assert dr.grow_window((10, 20, 30, 40), 5, 90, 120) == (5, 15, 35, 45)
    assert dr.grow_window((2, 3, 118, 88), 32, 90, 120) == (0, 0, 120, 90)
    assert dr.grow_window((0, 0, 0, 0), 32, 90, 120) == (0, 0, 0, 0) and dr.grow_window((5, 5, 5, 9), 4, 90, 120) == (0, 0, 0, 0)
    scene, _, poses, wins = do.mixed()
    obj = scn.obj_index(m, scene["obj_ids"])
    nan_pose = np.stack(poses).copy()
    nan_pose[3, 0, 0] = np.nan
    nan_pose[4, :3, 3] = (5000.0, 0, 500.0)                       # off-frame
    windows, groups = dr.plan_views(m, obj, scene["image_index"], nan_pose, vo.CAMS, vo.H, vo.W, 1.0, 32, 1 << 30)
    assert len(groups) == 1 and groups[0].tolist() == list(range(len(obj)))
    for p in range(len(obj)):
        want = (0, 0, 0, 0) if p in (3, 4) else wins[p]
        assert tuple(windows[p]) == want, (p, windows[p], want)   # the oracle's plan and the module's agree
    tight, _ = dr.plan_views(m, obj, scene["image_index"], np.stack(poses), vo.CAMS, vo.H, vo.W, 1.0, 0, 1 << 30)
    inside = (tight[:, 2] > tight[:, 0])
    assert np.all(windows[[0, 1, 2]][:, :2] <= tight[[0, 1, 2]][:, :2]) and np.all(windows[[0, 1, 2]][:, 2:] >= tight[[0, 1, 2]][:, 2:]) and inside.all()
    _, small = dr.plan_views(m, obj, scene["image_index"], np.stack(poses), vo.CAMS, vo.H, vo.W, 1.0, 32, 60000)
    assert len(small) > 2 and np.concatenate(small).tolist() == list(range(len(obj)))
    _, single = dr.plan_views(m, obj, scene["image_index"], np.stack(poses), vo.CAMS, vo.H, vo.W, 1.0, 32, 1)
    assert [g.tolist() for g in single] == [[p] for p in range(len(obj))]
    off = dr.strip_offsets(np.array([[0, 0, 10, 8], [0, 0, 10, 9], [0, 0, 0, 0], [3, 3, 3, 20], [5, 7, 6, 8]], dtype=np.int32))
    assert off.tolist() == [0, 1, 3, 3, 3, 4] and off.dtype == np.int32
    assert dr._boxes(m).shape == (3, 6) and np.array_equal(dr._boxes(m)[0], F([-40, -40, -40, 40, 40, 40]))


def _canned(status, rms):
    """refine_poses_depth's result for canned poses: R = identity, t = (n, 0, 500 + n) for pose n."""
    import torch

    n = len(status)
    return {"R": torch.eye(3).repeat(n, 1, 1), "t": torch.tensor([[k, 0.0, 500.0 + k] for k in range(n)]),
            "status": torch.tensor(status, dtype=torch.int32), "rms_after": torch.tensor(rms, dtype=torch.float32)}


def _preds():
    hyp = lambda r, z: {"R_stage_3": np.eye(3).reshape(9), "t_stage_3": np.array([0.0, 0.0, z]), "inliers_ratio": r}  # noqa: E731
    return [[hyp(0.9, 400.0), hyp(0.8, 410.0), hyp(0.7, 420.0)], [hyp(0.6, 430.0), hyp(0.5, 440.0)]]


def test_refine_predictions_ranking_validation_and_csv_stage(monkeypatch):
    m = _cpu_models()
    K, d = np.array([[100.0, 0, 60], [0, 100.0, 45], [0, 0, 1]]), np.zeros((vo.H, vo.W), dtype=F)
    calls = []

    def fake(models, ids, R, t, K_, depth, depth_scale=None, **kw):
        calls.append((np.asarray(ids).tolist(), np.asarray(t)[:, 2].tolist(), tuple(depth.shape), kw))
        table = {5: ([1, 3, 0, 0, 2], [5.0, 0.1, 2.0, 1.0, 0.5]), 2: ([0, 2], [3.0, 4.0])}[len(ids)]
        return _canned(*table)

    monkeypatch.setattr(dr, "refine_poses_depth", fake)
    preds = _preds()
    best = pipeline.refine_predictions(preds, m, [1, 2], K, d, iterations=3)
    assert calls[-1] == ([1, 2], [400.0, 430.0], (1, vo.H, vo.W), {"iterations": 3})            # one call, the best hypotheses only
    assert "R_depth" not in preds[0][0] and "R_depth" not in best[0][1] and best[0][0]["depth_status"] == 0 and best[1][0]["depth_status"] == 2
    assert best[1][0]["t_depth"].tolist() == [1.0, 0.0, 501.0] and best[0][0]["R_depth"].shape == (9,) and best[1][0]["depth_rms"] == 4.0
    every = pipeline.refine_predictions(preds, m, [1, 2], K, d[None], hypotheses="all")
    assert calls[-1][0] == [1, 1, 1, 2, 2] and [h["inliers_ratio"] for h in every[0]] == [0.9, 0.8, 0.7]
    ranked = pipeline.refine_predictions(preds, m, [1, 2], K, d, hypotheses="all", rank_by="depth")
    # instance 0: statuses (1, 3, 0), rms (5, 0.1, 2): the valid ones by rms, then the rejected one; instance 1: (0, 2), rms (1, 0.5)
    assert [h["inliers_ratio"] for h in ranked[0]] == [0.7, 0.9, 0.8] and [h["inliers_ratio"] for h in ranked[1]] == [0.6, 0.5]
    assert len(calls) == 3
    for kw in ({"hypotheses": "first"}, {"rank_by": "rms"}, {"rank_by": "depth"}, {"obj_ids": [1]}, {"depth": np.zeros((2, vo.H, vo.W), dtype=F)},
               {"depth": np.zeros(5, dtype=F)}):
        with pytest.raises(ValueError):
            pipeline.refine_predictions(**dict(dict(preds_image=preds, models=m, obj_ids=[1, 2], K=K, depth=d), **kw))
    assert len(calls) == 3
    # the results rows: the default is the old output byte for byte, "depth" writes the refined pose of the best hypothesis
    old = pipeline.bop_csv_lines(3, 7, [1, 2], [0.5, 0.25], preds, 1.5)
    assert pipeline.bop_csv_lines(3, 7, [1, 2], [0.5, 0.25], every, 1.5, stage="stage_3") == old and old[0].startswith("3,7,1,0.5,1.0 0.0")
    assert pipeline.bop_csv_lines(3, 7, [1, 2], [0.5, 0.25], best, 1.5) == old
    rows = ev.read_bop_results(pipeline.bop_csv_lines(3, 7, [1, 2], [0.5, 0.25], ranked, 1.5, stage="depth"))
    assert rows["t"].tolist() == [[2.0, 0.0, 502.0], [3.0, 0.0, 503.0]] and rows["obj_id"].tolist() == [1, 2] and rows["time"].tolist() == [1.5, 1.5]
    with pytest.raises(ValueError):
        pipeline.bop_csv_lines(3, 7, [1, 2], [0.5, 0.25], preds, 1.5, stage="depth")           # not refined
    with pytest.raises(ValueError):
        pipeline.bop_csv_lines(3, 7, [1, 2], [0.5, 0.25], best, 1.5, stage="stage_2")


def test_depth_refine_abi_argument_validation_needs_no_gpu():
    from picopose_amd import _lib

    L = _lib.lib()
    assert {"pp_depth_refine", "pp_depth_refine_workspace_bytes"} <= set(_lib.declared_symbols())
    need = ctypes.c_size_t()
    assert L.pp_depth_refine_workspace_bytes(1000, 24, 13, ctypes.byref(need)) == 0 and need.value == 256 + 8192 + 256 + 13 * 232
    assert L.pp_depth_refine_workspace_bytes(0, 24, 0, ctypes.byref(need)) == 0 and need.value == 256 + 256
    for args in ((-1, 24, 0), (10, 0, 1), (10, 2 ** 32, 1), (2 ** 62, 1, 1), (10, 5, -1), (10, 5, 11), (2 ** 40, 5, 2 ** 31)):
        assert L.pp_depth_refine_workspace_bytes(*args, ctypes.byref(need)) == -1, args
    assert L.pp_depth_refine_workspace_bytes(10, 10, 1, None) == -1
    buf, p = st.aligned_buffer()
    i32, f32, i64 = st.i32, st.f32, st.i64
    scene = dict(st.fields(p), poses=p + 4096)                     # (the input poses must not be poses_out)
    ws_bytes = 256 + 1792 + 256 + 4 * 232
    own = dict(boxes=p, boxes_host=f32(-1, -1, -1, 1, 1, 1, 0, 0, 0, 2, 2, 0), view_soff=p, view_soff_host=i32(0, 2, 4, 4), depth=p, iterations=10,
               max_distance=100.0, min_points=1000, min_cos=0.1, rcond=1e-6, eps=1e-2, max_translation=100.0, max_rotation=0.5, workspace=p,
               workspace_bytes=ws_bytes, poses_out=p, active=p, status=p, n_iterations=p, rank=p, n_points=p, rms_before=p, rms_after=p,
               near_count=p, trajectory=None, sums=None)
    call = st.caller(L.pp_depth_refine, scene, own)

    # (a valid argument list would launch: it is never sent here; every call below differs from it in one invalid argument)
    assert call(scene=None) == -1
    pointers = list(st.DEVICE_TABLES) + [k for k in own if own[k] is p and k != "workspace"]
    assert len(pointers) == 23
    for k in pointers:
        assert call(**{k: None}) == -1, k
    for k in st.HOST_TABLES + ("boxes_host", "view_soff_host", "workspace"):
        assert call(**{k: None}) == -1, k
    nan, inf = float("nan"), float("inf")
    for kw in ({"poses": p}, {"n_objects": 0}, {"n_images": 0}, {"n_views": 0}, {"H": 0}, {"W": -3}, {"H": 50000, "W": 50000}, {"iterations": 0},
               {"iterations": 1001}, {"max_distance": 0.0}, {"max_distance": inf}, {"max_distance": nan}, {"min_points": 0}, {"min_points": -5},
               {"min_cos": -0.5}, {"min_cos": 1.0}, {"min_cos": nan}, {"rcond": -1.0}, {"rcond": 1.0}, {"rcond": nan}, {"eps": -1.0}, {"eps": inf},
               {"eps": nan}, {"max_translation": 0.0}, {"max_translation": nan}, {"max_rotation": -0.5}, {"max_rotation": inf}, {"near": 0.0},
               {"near": inf}, {"diameters_host": f32(100.0, 0.0)}, {"boxes_host": f32(-1, -1, -1, 1, 1, 1, 0, 0, 0, 2, 2, -1)},
               {"boxes_host": f32(-1, nan, -1, 1, 1, 1, 0, 0, 0, 2, 2, 0)}, {"cams_host": f32(0, 100, 32, 24, 90, 95, 30, 20)},
               {"vert_off_host": i32(1, 4, 7)}, {"face_off_host": i32(0, 3, 3)}, {"faces_host": i32(0, 1, 2, 0, 2, 4, 0, 1, 2)},
               {"view_obj_host": i32(0, 2, 1)}, {"view_img_host": i32(0, -1, 1)}, {"windows_host": i32(0, 0, 10, 10, 55, 38, 65, 48, 5, 5, 5, 9)},
               {"view_zoff_host": i64(0, 100, 200, 201)}, {"view_soff_host": i32(0, 2, 4, 5)}, {"view_soff_host": i32(0, 1, 3, 3)},
               {"view_soff_host": i32(1, 3, 5, 5)}):
        assert call(**kw) == -1, kw
    # PP_EWORKSPACE.  These calls pass every check of the scene before they fail on the workspace, so they are also the guard that the
    # ctypes layout of _lib.PpScene is the C struct's.
    assert call(workspace_bytes=ws_bytes - 1) == -2 and call(workspace=p + 64) == -2 and call(workspace_bytes=0) == -2


def test_scene_tables_get_the_same_code_from_pp_vsd_errors_and_pp_depth_refine_needs_no_gpu():
    """The object, camera and view tables are validated once for the three entries that take a PpScene: each malformed table below, with
    everything else well formed, gets PP_EINVAL from pp_vsd_errors, pp_depth_refine and pp_scene_gt (pad (0, 0): the canvas is the
    frame), all three reading ONE struct instance, and a workspace one byte short or misaligned PP_EWORKSPACE from all three."""
    from picopose_amd import _lib

    L = _lib.lib()
    buf, p = st.aligned_buffer()
    i32, f32, i64 = st.i32, st.f32, st.i64
    nan, inf = float("nan"), float("inf")
    vsd_ws, refine_ws = 256 + 1792 + 5 * 8, 256 + 1792 + 256 + 4 * 232

    def three(ws=p, short=0, **kw):
        s = st.pack(dict(st.fields(p), poses=p + 4096, **kw))
        sc = ctypes.byref(s)
        vsd = L.pp_vsd_errors(sc, p, p, i32(0, 2), i32(1, 2), 2, p, 15.0, f32(0.1, 0.2), 2, ws, vsd_ws - short, p, p, p, None, None)
        refine = L.pp_depth_refine(sc, p, f32(-1, -1, -1, 1, 1, 1, 0, 0, 0, 2, 2, 0), p, i32(0, 2, 4, 4), p, 10, 100.0, 1000, 0.1, 1e-6, 1e-2,
                                   100.0, 0.5, ws, refine_ws - short, p, p, p, p, p, p, p, p, p, None, None, None)
        gt = L.pp_scene_gt(sc, p, s.keep["cams_host"], 0, 0, p, 15.0, None, 0, ws, vsd_ws - short, p, p, p, None, None, None, None, None)
        return vsd, refine, gt

    # (the well-formed call would launch: it is never sent; every call below differs from it in one table or in the workspace)
    cases = {"vert_off[0] != 0": {"vert_off_host": i32(1, 4, 7)}, "non-increasing vert_off": {"vert_off_host": i32(0, 4, 4)},
             "face index == vertex count": {"faces_host": i32(0, 1, 2, 0, 2, 4, 0, 1, 2)}, "diameter 0": {"diameters_host": f32(100.0, 0.0)},
             "diameter inf": {"diameters_host": f32(inf, 50.0)}, "diameter NaN": {"diameters_host": f32(100.0, nan)},
             "fx == 0": {"cams_host": f32(0, 100, 32, 24, 90, 95, 30, 20)}, "non-finite cx": {"cams_host": f32(100, 100, 32, 24, 90, 95, inf, 20)},
             "view_obj out of range": {"view_obj_host": i32(0, 2, 1)}, "view_img out of range": {"view_img_host": i32(0, -1, 1)},
             "an object of the call without faces": {"face_off_host": i32(0, 3, 3)},
             "x1 > W": {"windows_host": i32(0, 0, 10, 10, 55, 38, 65, 48, 5, 5, 5, 9)},
             "inverted window": {"windows_host": i32(0, 0, 10, 10, 54, 38, 64, 48, 6, 5, 5, 9)},
             "view_zoff[0] != 0": {"view_zoff_host": i64(1, 101, 201, 201)}, "view_zoff step is not the area": {"view_zoff_host": i64(0, 100, 200, 201)}}
    assert len(cases) == 15
    for name, kw in cases.items():
        assert three(**kw) == (-1, -1, -1), name                             # PP_EINVAL
    assert three(short=1) == (-2, -2, -2) and three(ws=p + 8) == (-2, -2, -2)      # PP_EWORKSPACE: one byte short, misaligned by 8
