"""CPU: the pose-error oracle (tests/pose_error_oracle.py) and the host layer of picopose_amd/evaluation.py against closed forms."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_error_oracle as po  # noqa: E402

from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd.pipeline import bop_csv_lines  # noqa: E402

H = 40.0
CUBE = np.array([[x, y, z] for x in (-H, H) for y in (-H, H) for z in (-H, H)])
CUBE_INFO = {"diameter": 2 * H * math.sqrt(3), "symmetries_discrete": po.cube_symmetries()}
ROT90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])        # exact entries: products with it do not round
K = np.array([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]])


def _both(V, syms, Re, te, Rg, tg, K_=K, **kw):
    """The float64 definitions and the float32 restatement of the kernel on the same pair."""
    syms = np.asarray(syms, dtype=np.float64)
    a = po.errors64(V, syms, Re, te, Rg, tg, K_, **kw)
    b = po.errors32(np.asarray(V, dtype=np.float32), syms[:, :3, :3].reshape(-1, 9), syms[:, :3, 3], Re, te, Rg, tg, K_[0, 0], K_[1, 1], **kw)
    return a, b


def test_pure_translation_and_identical_poses():
    V = np.array([[10.0, 0, 0], [0, 20, 0], [0, 0, 30], [-5, -5, -5]])
    t = np.array([0.0, 0.0, 500.0])
    for res in _both(V, np.eye(4)[None], np.eye(3), t + [3.0, 4.0, 12.0], np.eye(3), t):
        assert res["mssd"] == 13.0 and res["add"] == 13.0 and res["adds"] <= 13.0
    for res in _both(V, np.eye(4)[None], ROT90, t, ROT90, t):
        assert res["mssd"] == 0 and res["mspd"] == 0 and res["add"] == 0 and res["adds"] == 0


def test_cube_with_its_24_rotations():
    syms = ev.symmetry_transforms(CUBE_INFO)
    assert syms.shape == (24, 4, 4) and np.array_equal(syms[0], np.eye(4))
    assert np.array_equal(syms, po.symmetry_set(CUBE_INFO))
    assert len({tuple(s[:3, :3].round().astype(int).ravel()) for s in syms}) == 24
    Rg, tg = ROT90, np.array([10.0, -20.0, 600.0])
    for k, S in enumerate(syms):
        for res in _both(CUBE, syms, Rg @ S[:3, :3], tg, Rg, tg):
            assert res["mssd"] == 0 and res["mspd"] == 0 and res["mssd_sym"] == k and res["mspd_sym"] == k
            assert res["adds"] == 0                               # a symmetry that permutes the vertices
    # without the symmetries: a half turn about z moves every vertex (x, y, z) to (-x, -y, z), 2 sqrt(2) H away
    Rz = np.diag([-1.0, -1.0, 1.0])
    for res in _both(CUBE, np.eye(4)[None], Rg @ Rz, tg, Rg, tg):
        assert res["mssd"] == pytest.approx(2 * math.sqrt(2) * H, rel=1e-6) and res["add"] == pytest.approx(2 * math.sqrt(2) * H, rel=1e-6)
        assert res["adds"] == 0 and res["mssd_sym"] == 0


def test_product_order_of_a_discrete_and_a_continuous_symmetry_by_hand():
    """One discrete symmetry D (half turn about x, then 4 mm along z) and one continuous symmetry about z through (1, 2, 0), at a step of
    pi / 4: ceil(pi / (pi / 4)) = 4 rotations C_k by k 90 degrees, x -> R (x - off) + off, i.e. t = off - R off:
      C_1: R = [[0,-1,0],[1,0,0],[0,0,1]], R off = (-2, 1, 0), t = (3, 1, 0);   C_2: R = diag(-1,-1,1), t = (2, 4, 0).
    Rows are discrete-major, T = C_k D: rows 0..3 = C_k, rows 4..7 = C_k D.
      row 5 = C_1 D: R = C_1 diag(1,-1,-1) = [[0,1,0],[1,0,0],[0,0,-1]], t = C_1 (0,0,4) + (3,1,0) = (3, 1, 4);
      row 6 = C_2 D: R = diag(-1,-1,1) diag(1,-1,-1) = diag(-1,1,-1), t = (0,0,4) + (2,4,0) = (2, 4, 4)."""
    D = [1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 4, 0, 0, 0, 1]
    info = {"diameter": 1.0, "symmetries_discrete": [D], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [1, 2, 0]}]}
    T = ev.symmetry_transforms(info, max_sym_disc_step=math.pi / 4)
    assert T.shape == (8, 4, 4)
    want = {0: np.eye(4),
            1: [[0, -1, 0, 3], [1, 0, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]],
            2: [[-1, 0, 0, 2], [0, -1, 0, 4], [0, 0, 1, 0], [0, 0, 0, 1]],
            4: np.array(D, dtype=float).reshape(4, 4),
            5: [[0, 1, 0, 3], [1, 0, 0, 1], [0, 0, -1, 4], [0, 0, 0, 1]],
            6: [[-1, 0, 0, 2], [0, 1, 0, 4], [0, 0, -1, 4], [0, 0, 0, 1]]}
    for k, w in want.items():
        assert np.allclose(T[k], np.array(w, dtype=float), atol=1e-12), (k, T[k])
    assert np.allclose(po.symmetry_set(info, math.pi / 4), T, atol=1e-12)


def test_a_non_finite_pose_is_infinitely_wrong_in_the_oracle_and_never_matched():
    V = np.array([[10.0, 0, 0], [0, 20, 0], [0, 0, 30], [-5, -5, -5]])
    t = np.array([0.0, 0.0, 500.0])
    for bad_t, bad_R in ((np.array([np.nan, 0, 500.0]), np.eye(3)), (t, np.diag([np.inf, 1, 1])), (np.array([0, np.inf, 500.0]), np.eye(3))):
        for est_side in (True, False):
            a = (bad_R, bad_t, np.eye(3), t) if est_side else (np.eye(3), t, bad_R, bad_t)
            with np.errstate(invalid="ignore", over="ignore"):
                for res in _both(V, np.eye(4)[None], *a):
                    assert res["mssd"] == np.inf and res["mspd"] == np.inf and res["mssd_sym"] == 0, res
                    assert not np.isfinite(res["add"]) and not np.isfinite(res["adds"]), res
    # +inf and NaN errors are below no limit: the estimate is not matched, whatever its score
    pairs = {"target": np.array([0, 0]), "est": np.array([0, 1]), "gt": np.array([0, 0])}
    models = ev.ObjectModels({5: {"vertices": V, "info": {"diameter": 20.0}}}, device="cpu")
    for bad in (np.inf, np.nan):
        res = ev.score_errors(pairs, [bad, 0.25], [bad, 1.0], np.array([0.9, 0.1]), np.array([[1, 2, 5, 2]]), models)
        assert res["recall_mssd"].tolist() == [0.5] * 10 and res["recall_mspd"].tolist() == [0.5] * 10


def test_continuous_symmetry_of_a_ring():
    r, off = 35.0, np.array([12.0, -7.0, 0.0])
    info = {"diameter": 2 * r, "symmetries_continuous": [{"axis": [0, 0, 2.0], "offset": off.tolist()}]}
    syms = ev.symmetry_transforms(info)
    n = int(math.ceil(math.pi / 0.01))
    assert n == 315 and syms.shape == (315, 4, 4) and np.allclose(syms, po.symmetry_set(info), atol=1e-12)
    for k, T in enumerate(syms):
        R = T[:3, :3]
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.allclose(R @ [0, 0, 1.0], [0, 0, 1.0], atol=1e-12)
        assert np.allclose(T[:3, :3] @ off + T[:3, 3], off, atol=1e-12)                      # the axis passes through the offset
        assert math.atan2(R[1, 0], R[0, 0]) % (2 * math.pi) == pytest.approx(2 * math.pi * k / n, abs=1e-12)
    ang = np.linspace(0, 2 * math.pi, 90, endpoint=False)
    V = np.concatenate([np.stack([r * np.cos(ang), r * np.sin(ang), np.full(90, z)], axis=1) for z in (-10.0, 0.0, 25.0)]) + off
    # the nearest discrete step is at most half a step (pi / 315) away: every vertex then moves by a chord of that angle at most
    bound = 2 * r * math.sin(math.pi / n / 2)
    rng = np.random.default_rng(0)
    Rg, tg = po.random_rotation(rng), np.array([30.0, 40.0, 700.0])
    for a in (0.0123, 1.0, 2.2222, 5.9):
        T = np.eye(4)
        T[:3, :3] = po.axis_rotation([0, 0, 1.0], a)
        T[:3, 3] = off - T[:3, :3] @ off
        a64, a32 = _both(V, syms, Rg @ T[:3, :3], Rg @ T[:3, 3] + tg, Rg, tg)
        assert a64["mssd"] <= bound * (1 + 1e-9)
        assert a32["mssd"] <= bound + po.metric_bound(po.max_norm(V, syms), tg, tg)
        assert po.errors64(V, np.eye(4)[None], Rg @ T[:3, :3], Rg @ T[:3, 3] + tg, Rg, tg, K, kinds=("mssd",))["mssd"] > bound


def test_mspd_of_a_fronto_parallel_shift():
    V = np.array([[10.0, 5, 0], [-20, 8, 0], [3, -30, 0], [0, 0, 0]])                      # a planar object facing the camera
    z, d = 800.0, np.array([6.0, -8.0, 0.0])
    a64, a32 = _both(V, np.eye(4)[None], np.eye(3), [0, 0, z] + d, np.eye(3), [0, 0, z])
    assert a64["mspd"] == pytest.approx(600.0 * 10.0 / z, rel=1e-12) and float(a32["mspd"]) == pytest.approx(600.0 * 10.0 / z, rel=1e-6)
    # a point at or behind the camera plane: +inf, not NaN
    for res in _both(V, np.eye(4)[None], np.eye(3), [0, 0, 0.0], np.eye(3), [0, 0, z]):
        assert res["mspd"] == np.inf


def test_adds_never_exceeds_add():
    rng = np.random.default_rng(1)
    V = rng.uniform(-50, 50, (300, 3))
    for _ in range(5):
        Rg, tg = po.random_rotation(rng), np.array([0, 0, 900.0])
        a64, a32 = _both(V, np.eye(4)[None], Rg @ po.random_rotation(rng, 0.5), tg + rng.normal(size=3) * 5, Rg, tg)
        assert a64["adds"] <= a64["add"] and a32["adds"] <= a32["add"]
        for k in ("mssd", "add", "adds"):
            assert abs(float(a32[k]) - a64[k]) <= po.metric_bound(po.max_norm(V, np.eye(4)[None]), tg, tg)


def test_kd_tree_and_brute_force_nearest_neighbours_agree(monkeypatch):
    rng = np.random.default_rng(2)
    V = rng.uniform(-50, 50, (1500, 3)).astype(np.float32)
    V[100] = V[7]                                                 # a duplicated vertex: exact ties
    Rg, tg = po.random_rotation(rng), np.array([0, 0, 900.0])
    Re, te = Rg @ po.random_rotation(rng, 0.05), tg + [1.0, 2.0, -1.0]
    brute = [f(V, *a, kinds=("adds",))["adds"] for f, a in ((po.errors64, (np.eye(4)[None], Re, te, Rg, tg)),
                                                             (po.errors32, (np.eye(3).reshape(1, 9), np.zeros((1, 3)), Re, te, Rg, tg)))]
    monkeypatch.setattr(po, "BRUTE", 10)
    assert po.errors64(V, np.eye(4)[None], Re, te, Rg, tg, kinds=("adds",))["adds"] == pytest.approx(brute[0], rel=1e-13)
    assert po.errors32(V, np.eye(3).reshape(1, 9), np.zeros((1, 3)), Re, te, Rg, tg, kinds=("adds",))["adds"] == brute[1]


def test_mspd_bound_holds_for_the_gpu_suites_inputs():
    """The float32 restatement stays inside mspd_bound (c = 48, derived in its docstring) of the float64 definitions on every pair of the
    GPU suite's mixed call, and those inputs keep z_min >= |t| / 4 so that the bound says something."""
    objects, pairs = po.mixed_inputs()
    models = ev.ObjectModels(objects, device="cpu")
    worst = 0.0
    for i, o in enumerate(pairs["obj_ids"].tolist()):
        k = models.index[o]
        s0, s1 = models.sym_off[k], models.sym_off[k + 1]
        syms = np.tile(np.eye(4), (s1 - s0, 1, 1))
        syms[:, :3, :3], syms[:, :3, 3] = models.sym_R_host[s0:s1].reshape(-1, 3, 3), models.sym_t_host[s0:s1]
        V = objects[o]["vertices"]
        a = [pairs[n][i].astype(np.float64) for n in ("R_est", "t_est", "R_gt", "t_gt")]
        Kp = pairs["K"][i].astype(np.float64)
        e64 = po.errors64(V, syms, *a, Kp, kinds=("mspd",))
        e32 = po.errors32(V, models.sym_R_host[s0:s1], models.sym_t_host[s0:s1], *a, Kp[0, 0], Kp[1, 1], kinds=("mspd",))
        zmin = po.min_depth(V, syms, *a)
        assert zmin >= max(np.linalg.norm(a[1]), np.linalg.norm(a[3])) / 4
        bound = po.mspd_bound(po.max_norm(V, syms), a[1], a[3], max(Kp[0, 0], Kp[1, 1]), zmin)
        assert abs(float(e32["mspd"]) - e64["mspd"]) <= bound, (i, o, e32["mspd"], e64["mspd"], bound)
        worst = max(worst, abs(float(e32["mspd"]) - e64["mspd"]) / bound)
    print(f"largest |mspd32 - mspd64| / bound over {len(pairs['obj_ids'])} pairs: {worst:.3f}")


def test_parsers_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    preds = [[{"R_stage_3": po.random_rotation(rng).astype(np.float32).reshape(9), "t_stage_3": (rng.normal(size=3) * 300).astype(np.float32),
               "inliers_ratio": 0.5}] for _ in range(3)]
    scores = [np.float32(0.91), 0.5, np.float32(1 / 3)]
    lines = bop_csv_lines(48, 7, [1, 5, 5], scores, preds, 0.25)
    for src in (lines, ["scene_id,im_id,obj_id,score,R,t,time\n"] + lines):
        got = ev.read_bop_results(src)
        assert got["scene_id"].tolist() == [48] * 3 and got["im_id"].tolist() == [7] * 3 and got["obj_id"].tolist() == [1, 5, 5]
        assert got["time"].tolist() == [0.25] * 3 and got["score"].tolist() == [float(str(s)) for s in scores]
        for k, p in enumerate(preds):
            assert got["R"][k].ravel().tolist() == [float(str(v)) for v in p[0]["R_stage_3"]]
            assert got["t"][k].tolist() == [float(str(v)) for v in p[0]["t_stage_3"]]
            assert np.array_equal(got["R"][k].astype(np.float32).ravel(), p[0]["R_stage_3"])     # str() of a float32 round-trips
    path = tmp_path / "res.csv"
    path.write_text("".join(lines))
    assert np.array_equal(ev.read_bop_results(path)["R"], got["R"])
    with pytest.raises(ValueError):
        ev.read_bop_results(["1,2,3,0.5,1 0 0 0 1 0 0 0,0 0 0,0.1\n"])
    gt = {"3": [{"cam_R_m2c": list(range(9)), "cam_t_m2c": [1.5, 2, 3], "obj_id": 5}, {"cam_R_m2c": [0] * 9, "cam_t_m2c": [0, 0, 1], "obj_id": 1}],
          "10": []}
    cam = {"3": {"cam_K": [600, 0, 320, 0, 601, 240, 0, 0, 1], "depth_scale": 0.1}, "10": {"cam_K": [1, 0, 0, 0, 1, 0, 0, 0, 1]}}
    tg = [{"im_id": 3, "inst_count": 2, "obj_id": 5, "scene_id": 48}, {"im_id": 10, "inst_count": 1, "obj_id": 1, "scene_id": 48}]
    info = {"1": CUBE_INFO, "5": {"diameter": 10.5}}
    for name, obj in (("scene_gt.json", gt), ("scene_camera.json", cam), ("targets.json", tg), ("models_info.json", info)):
        (tmp_path / name).write_text(json.dumps(obj))
    g = ev.read_scene_gt(tmp_path / "scene_gt.json")
    assert sorted(g) == [3, 10] and g[3]["obj_id"].tolist() == [5, 1] and g[3]["R"][0].tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    assert g[3]["t"].tolist() == [[1.5, 2, 3], [0, 0, 1]] and g[10]["R"].shape == (0, 3, 3)
    c = ev.read_scene_camera(tmp_path / "scene_camera.json")
    assert c[3]["K"].tolist() == [[600, 0, 320], [0, 601, 240], [0, 0, 1]] and c[3]["depth_scale"] == 0.1 and c[10]["depth_scale"] == 1.0
    assert ev.read_targets(tmp_path / "targets.json").tolist() == [[48, 3, 5, 2], [48, 10, 1, 1]]
    with open(tmp_path / "models_info.json") as fh:
        assert ev.symmetry_transforms(json.load(fh)["1"]).shape == (24, 4, 4)


def test_greedy_matching_differs_from_the_best_assignment():
    """One image, two instances of object 5 at x = 0 (G0) and x = 7 (G1), diameter 20: the MSSD limits are 1, 2, ... 10 mm.
    Estimates (pure translations, so MSSD = the shift): A at x = 3, score 0.9: 3 mm from G0, 4 mm from G1.  B at x = -4.5, score 0.8:
    4.5 mm from G0, 11.5 mm from G1.  C at x = 7 (exactly G1), score 0.1: dropped, inst_count = 2 keeps A and B.
      limits 1, 2, 3: A is not BELOW any limit (3 < 3 fails), B neither: 0 of 2.
      limit 4: A takes G0 (3 < 4; 4 < 4 fails for G1); B has G0 taken and G1 too far: 1 of 2.
      limits 5 .. 10: A takes G0, its lowest error; B is within 4.5 of G0 but G0 is used, G1 is 11.5 away: 1 of 2 — the best
      assignment (A -> G1, B -> G0) would score 2 of 2.
    Recall = [0, 0, 0, .5, .5, .5, .5, .5, .5, .5], AR_MSSD = 0.35."""
    V = np.array([[5.0, 0, 0], [0, 5, 0], [0, 0, 5], [-5, -5, -5]])
    z = 500.0
    est = {"scene_id": np.array([1, 1, 1]), "im_id": np.array([2, 2, 2]), "obj_id": np.array([5, 5, 5]), "score": np.array([0.1, 0.8, 0.9]),
           "R": np.tile(np.eye(3), (3, 1, 1)), "t": np.array([[7.0, 0, z], [-4.5, 0, z], [3.0, 0, z]])}
    gt = {1: {2: {"obj_id": np.array([9, 5, 5]), "R": np.tile(np.eye(3), (3, 1, 1)), "t": np.array([[0, 0, 1.0], [0.0, 0, z], [7.0, 0, z]])}}}
    targets = np.array([[1, 2, 5, 2]])
    pairs = ev.plan_pairs(est, gt, targets)
    assert pairs["est"].tolist() == [2, 2, 1, 1] and pairs["gt"].tolist() == [1, 2, 1, 2]
    errs = [po.errors64(V, np.eye(4)[None], est["R"][e], est["t"][e], gt[1][2]["R"][g], gt[1][2]["t"][g], K, kinds=("mssd", "mspd"))
            for e, g in zip(pairs["est"], pairs["gt"])]
    assert [e["mssd"] for e in errs] == [3.0, 4.0, 4.5, 11.5]
    models = ev.ObjectModels({5: {"vertices": V, "info": {"diameter": 20.0}}}, device="cpu")
    res = ev.score_errors(pairs, [e["mssd"] for e in errs], [e["mspd"] for e in errs], est["score"], targets, models)
    want = [0, 0, 0, .5, .5, .5, .5, .5, .5, .5]
    assert res["recall_mssd"].tolist() == want and res["AR_MSSD"] == pytest.approx(0.35) and res["vsd"] is None and "AR" not in res
    assert res["per_object"][5]["recall_mssd"].tolist() == want and res["n_targets"] == 2
    # MSPD = 600 * shift / 500 px: 3.6, 4.8, 5.4, 13.8 against 5, 10, ... 50 px: A takes G0 at every limit; B reaches G1 from 15 px on
    assert res["recall_mspd"].tolist() == [.5, .5, 1, 1, 1, 1, 1, 1, 1, 1]
    ests = [{"scene": 1, "im": 2, "obj": 5, "score": s, "pose": (R, t)} for s, R, t in zip(est["score"], est["R"], est["t"])]
    gts = {(1, 2): [{"obj": int(o), "pose": (R, t)} for o, R, t in zip(gt[1][2]["obj_id"], gt[1][2]["R"], gt[1][2]["t"])]}
    rec, per_obj, _ = po.greedy_recalls(ests, gts, [(1, 2, 5, 2)], lambda o, a, b, s, i: po.errors64(V, np.eye(4)[None], *a, *b, kinds=("mssd",))["mssd"],
                                        lambda o, k: 20.0 * (k + 1) / 20.0, 10)
    assert rec.tolist() == want and per_obj[5].tolist() == want


def test_value_errors():
    for bad in ({"symmetries_discrete": [[1.0] * 15]}, {"symmetries_continuous": [{"axis": [0, 0, 0], "offset": [0, 0, 0]}]},
                {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, float("nan"), 0]}]},
                {"symmetries_discrete": [[float("inf")] * 16]}, {"symmetries_continuous": [{"axis": [0, 1], "offset": [0, 0, 0]}]}):
        with pytest.raises(ValueError):
            ev.symmetry_transforms(bad)
    with pytest.raises(ValueError):
        ev.ObjectModels({1: {"vertices": CUBE, "info": {}}}, device="cpu")                   # no diameter
    with pytest.raises(ValueError):
        ev.ObjectModels({1: {"vertices": CUBE[:, :2], "info": CUBE_INFO}}, device="cpu")
    models = ev.ObjectModels({1: {"vertices": CUBE, "info": CUBE_INFO}}, device="cpu")
    assert models.n_symmetries(1) == 24 and models.sym_R.shape == (24, 9) and models.vertices.dtype == torch.float32
    R, t = np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3))
    for kw in (dict(obj_ids=[1, 2]), dict(kinds=("mssd", "vsd")), dict(kinds=("mspd",), K=None), dict(R_est=R[:1]), dict(t_gt=np.zeros((2, 3, 1))),
               dict(R_gt=R.astype(np.int64)), dict(t_est=torch.zeros(2, 3, dtype=torch.int32)), dict(K=np.eye(4)), dict(obj_ids=[1.0, 1.0]), dict(K=np.eye(3, dtype=np.int64)), dict(K=[[1, 0], [0, 1]]), dict(R_est=[[1, 2], [3]]),
               dict(kinds=())):
        a = dict(obj_ids=[1, 1], R_est=R, t_est=t, R_gt=R, t_gt=t, K=K)
        a.update(kw)
        with pytest.raises(ValueError):
            ev.pose_errors(models, **a)
    out = ev.pose_errors(models, [], R[:0], t[:0], R[:0], t[:0], K=K, kinds=("mssd", "mspd", "add", "adds"))   # P = 0: no launch
    assert all(out[k].shape == (0,) for k in ("mssd", "mspd", "add", "adds", "mssd_sym", "mspd_sym")) and out["mssd_sym"].dtype == torch.int32
    sub = ev.ObjectModels({1: {"vertices": np.arange(30.0).reshape(10, 3), "info": {"diameter": 1.0}}}, max_points=4, device="cpu")
    assert sub.adds_vertices_host[:, 0].tolist() == [0.0, 9.0, 18.0, 27.0] and sub.vertices.shape == (10, 3)    # every ceil(10 / 4) = 3rd
