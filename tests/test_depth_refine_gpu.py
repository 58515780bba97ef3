"""GPU: pp_depth_refine (picopose_amd/depth_refine.py: refine_poses_depth; pipeline.refine_predictions) against
tests/depth_refine_oracle.py: the sums of one linearisation, every step of the trajectories teacher-forced through the oracle,
convergence onto the ground truth, the edge shapes and statuses, determinism across streams, pose order, batch composition and
grouping, and the path through the results rows into match_and_score's VSD."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_refine_oracle as do  # noqa: E402
import vsd_oracle as vo  # noqa: E402

from picopose_amd import depth_refine as dr  # noqa: E402  (absent before the feature)
from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import pipeline  # noqa: E402

gpu = pytest.mark.gpu
F = np.float32
OUT = ("R", "t", "status", "iterations", "rank", "n_points", "rms_before", "rms_after", "near_count")


def _np(r):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _mixed_call(models, rows=None, **kw):
    scene, _, poses, _ = do.mixed()
    rows = np.arange(len(poses)) if rows is None else np.asarray(rows)
    P = np.stack(poses)[rows]
    return _np(dr.refine_poses_depth(models, scene["obj_ids"][rows], P[:, :3, :3], P[:, :3, 3], scene["K"], scene["depth_u16"],
                                     image_index=scene["image_index"][rows], depth_scale=scene["depth_scale"], **dict(do.MIXED_PARAMS, **kw)))


def _conv_call(models, **kw):
    sc = do.convergence_scene()
    P = sc["start"]
    return _np(dr.refine_poses_depth(models, sc["obj_ids"], P[:, :3, :3], P[:, :3, 3], sc["K"], sc["depth_mm"], image_index=sc["image_index"],
                                     **dict(do.CONV_PARAMS, **kw)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _ulp(scale):
    return 2.0 ** (math.floor(math.log2(scale)) - 23)


@gpu
def test_one_linearisation_of_the_mixed_scene_equals_the_oracle_sums():
    """Cube, icosphere and plate under two cameras, uint16 depth with occluders and a missing block, ONE call, one iteration: N equals
    the oracle exactly, and every one of the 28 sums lies within 64 N 2^-53 sum|term| of the oracle's exactly rounded sum (the bound of
    a float64 summation of N terms in any order, with a factor for the rounding of the terms themselves).  fragile == 0 for this scene is
    asserted in test_depth_refine_cpu.py."""
    scene, dm, poses, wins = do.mixed()
    got = _mixed_call(ev.ObjectModels(scene["objects"]), iterations=1, debug=True)
    total = 0
    for p, o in enumerate(scene["obj_ids"].tolist()):
        im = int(scene["image_index"][p])
        sums, N, fragile, mag = do.linearise(poses[p], scene["objects"][o], vo.CAMS[im], dm[im], wins[p], return_abs=True)
        g = got["sums"][p, 0]
        err = np.abs(g - sums)
        print(f"pose {p} object {o}: N {N}, worst error / bound {np.max(err[:28] / np.maximum(64 * max(N, 1) * do.U64 * mag[:28], 1e-300)):.3g}")
        assert fragile == 0 and g[28] == N == got["n_points"][p], (p, g[28], N)
        assert np.all(err[:28] <= 64 * N * do.U64 * mag[:28]), (p, err, mag)
        assert got["iterations"][p] == 1 and (got["status"][p] == 2) == (N < do.MIXED_PARAMS["min_points"])
        total += N
    assert total > 2000 and got["n_groups"] == 1


@gpu
def test_every_step_of_the_trajectories_equals_the_oracle_step():
    """Teacher forcing: trajectory[k + 1] must be f32(oracle.step(oracle.linearise(trajectory[k]))) within 4 float32 ulps of the entry's
    scale (1 for the rotation, the largest |t| for the translation: the solver's own error, 1 / rcond 2^-53, is far below one ulp), for
    the mixed and the convergence scene.  Steps in which the oracle sees a fragile sample or an eigenvalue within 10 % of the rank
    cut are left out: at most 5 % of all steps.  The final status, iteration count, N and rank equal the oracle's on the last pose."""
    checked = skipped = 0
    for scene, got, params, poses in ((do.mixed()[0], None, do.MIXED_PARAMS, do.mixed()[2]), (do.convergence_scene(), None, do.CONV_PARAMS, None)):
        models = ev.ObjectModels(scene["objects"])
        if poses is not None:
            got, dm = _mixed_call(models, debug=True), do.mixed()[1]
        else:
            got, dm, poses = _conv_call(models, debug=True), scene["depth_mm"], list(scene["start"])
        for p, o in enumerate(scene["obj_ids"].tolist()):
            im, obj = int(scene["image_index"][p]), scene["objects"][o]
            win = do.plan(obj, poses[p], vo.CAMS[im], vo.H, vo.W)
            traj, iters, status = got["trajectory"][p], int(got["iterations"][p]), int(got["status"][p])
            assert np.array_equal(_bits(traj[0]), _bits(np.asarray(poses[p], dtype=F))) and iters >= 1
            for k in range(iters):
                sums, N, fragile = do.linearise(traj[k], obj, vo.CAMS[im], dm[im], win, params["max_distance"], params["min_cos"], params["near"])
                last = k == iters - 1
                if N < params["min_points"]:
                    assert last and status == 2 and np.array_equal(_bits(traj[k + 1]), _bits(traj[0]))
                    continue
                want, rank, info = do.step(sums, traj[k], obj, params["rcond"], full=True)
                if fragile or info["cut_margin"] < 0.1:
                    skipped += 1
                    continue
                checked += 1
                if last and status == 3:
                    dt, ang = do.drift(want, traj[0])
                    assert dt > params["max_translation"] or ang > params["max_rotation"], (p, k, dt, ang)
                    assert np.array_equal(_bits(traj[k + 1]), _bits(traj[0]))
                    continue
                tol = np.full((4, 4), 4 * _ulp(1.0))
                tol[:3, 3] = 4 * _ulp(float(np.abs(want[:3, 3]).max()))
                assert np.all(np.abs(traj[k + 1].astype(np.float64) - want.astype(np.float64)) <= tol), (p, k, traj[k + 1] - want)
                if last:
                    assert got["rank"][p] == rank and got["n_points"][p] == N, (p, got["rank"][p], rank)
                    small = max(np.linalg.norm(info["x"][:3]), np.linalg.norm(info["x"][3:])) < do.f32(params["eps"])
                    assert status == (0 if small else 1) and (small or iters == params["iterations"])
            assert all(np.array_equal(_bits(traj[k]), _bits(traj[iters])) for k in range(iters, params["iterations"] + 1))
            assert np.array_equal(_bits(traj[-1][:3, :3]), _bits(got["R"][p])) and np.array_equal(_bits(traj[-1][:3, 3]), _bits(got["t"][p]))
    print(f"{checked} steps checked, {skipped} left out")
    assert checked >= 30 and skipped <= 0.05 * (checked + skipped)


@gpu
def test_convergence_onto_the_ground_truth_render():
    """The test depth is the ground truths' render over a wall; the starts are 20 mm off along the ray (the cube also 3 degrees): the
    kernel's final MSSD is at most the oracle's plus 1e-3 mm (the oracle's is below a tenth of the start's: test_depth_refine_cpu.py)."""
    sc = do.convergence_scene()
    got = _conv_call(ev.ObjectModels(sc["objects"]))
    for p, r in enumerate(do.convergence_runs()):
        obj = sc["objects"][int(sc["obj_ids"][p])]
        final = do.mssd(obj, vo.pose(got["R"][p], got["t"][p]), sc["gt"][p])
        want = do.mssd(obj, r["pose"], sc["gt"][p])
        print(f"pose {p}: MSSD start {do.mssd(obj, sc['start'][p], sc['gt'][p]):.3f}, kernel {final:.5f}, oracle {want:.5f} mm; status {got['status'][p]}")
        assert got["status"][p] in (0, 1) and final <= want + 1e-3
        assert got["status"][p] == r["status"] and got["iterations"][p] == r["iterations"] and got["rank"][p] == r["rank"]
        assert abs(got["rms_after"][p] - r["rms_after"]) <= 1e-3 and got["rms_after"][p] < 0.1 * got["rms_before"][p]


def _edge_scene():
    """The plate under PLATE_K4 on four 61 x 83 images: flat at 520 mm, all missing, flat at 650 mm, flat at 1210 mm."""
    H, W = vo.PLATE_HW
    depth = np.stack([np.full((H, W), v, dtype=F) for v in (520.0, 0.0, 650.0, 1210.0)])
    depth[1, ::2] = -5.0                                          # negative and NaN are missing like zero
    depth[1, 1::4] = np.nan
    nan = vo.pose()
    nan[1, 2] = np.nan
    cx, cy = vo.PLATE_K4[2], vo.PLATE_K4[3]
    rows = [("facing", vo.pose(), 0), ("border", vo.pose(t=(-190.0, 0, vo.PLATE_Z)), 0),
            ("one_sample", vo.pose(t=((-2.5 - cx) * 40.0, (-2.5 - cy) * 40.0, 4000.0)), 0), ("off_frame", vo.pose(t=(5000.0, 0, vo.PLATE_Z)), 0),
            ("nan", nan, 0), ("missing", vo.pose(), 1), ("few", vo.pose(t=(0, 0, 1200.0)), 3), ("far", vo.pose(), 2)]
    p = vo.plate(vo.PLATE_N)
    obj = {"vertices": p["vertices"], "faces": p["faces"], "info": {"diameter": vo.PLATE_DIAMETER}}
    return obj, depth, rows, dict(do.DEFAULTS, margin=0, min_points=100, max_distance=200.0)


@gpu
def test_degenerate_and_edge_shapes_in_one_call():
    obj, depth, rows, params = _edge_scene()
    H, W = vo.PLATE_HW
    models = ev.ObjectModels({3: obj})
    K = vo.k33(np.array([vo.PLATE_K4], dtype=F))[0]
    P = np.stack([r[1] for r in rows])
    img = np.array([r[2] for r in rows], dtype=np.int32)
    got = _np(dr.refine_poses_depth(models, [3] * len(rows), P[:, :3, :3], P[:, :3, 3], K, depth, image_index=img, **params))
    name = {r[0]: k for k, r in enumerate(rows)}
    wins = [do.plan(obj, r[1], vo.PLATE_K4, H, W, margin=0) for r in rows]
    assert wins[name["one_sample"]] == (0, 0, 1, 1) and wins[name["border"]][0] == 0 and wins[name["border"]][2] < 20
    assert wins[name["off_frame"]] == (0, 0, 0, 0) and wins[name["nan"]] == (0, 0, 0, 0)
    for k, (label, pose, im) in enumerate(rows):
        r = do.run(pose, obj, vo.PLATE_K4, depth[im], wins[k], **params)
        print(label, "status", got["status"][k], "iterations", got["iterations"][k], "rank", got["rank"][k], "N", got["n_points"][k], "t", got["t"][k])
        assert (got["status"][k], got["iterations"][k], got["rank"][k], got["n_points"][k]) == (r["status"], r["iterations"], r["rank"], r["n_points"]), label
        if r["status"] >= 2:                                      # the input pose, bit for bit
            assert np.array_equal(_bits(got["R"][k]), _bits(pose[:3, :3])) and np.array_equal(_bits(got["t"][k]), _bits(pose[:3, 3])), label
        else:
            assert np.abs(got["t"][k] - r["pose"][:3, 3]).max() <= 1e-3 and np.abs(got["R"][k] - r["pose"][:3, :3]).max() <= 1e-6, label
    want = {"facing": 0, "border": None, "one_sample": 2, "off_frame": 4, "nan": 4, "missing": 2, "few": 2, "far": 3}
    for label, st in want.items():
        assert st is None or got["status"][name[label]] == st, (label, got["status"][name[label]])
    assert got["status"][name["border"]] in (0, 1) and 100 <= got["n_points"][name["border"]] < vo.PLATE_N ** 2
    k = name["facing"]
    assert got["rank"][k] == 3 and got["n_points"][k] == vo.PLATE_N ** 2 and abs(got["t"][k][2] - 520.0) < 1e-3 and abs(got["rms_before"][k] - 20) < 1e-3
    # unobservable: unchanged to one float32 ulp of the entry's scale, |t| = 520 for the translation and 1 for the rotation (half an ulp
    # below 1).  Not to the bit: the render of the flat plate is flat only to a float32 ulp of 500, so the first step tilts the plate by
    # some 1e-8 rad, and the directions that the second linearisation cannot see are tilted by as much against the input's.
    assert np.all(np.abs(got["t"][k][:2]) <= _ulp(520.0)) and np.abs(got["R"][k][[0, 1], [1, 0]]).max() <= 2.0 ** -24
    assert got["n_points"][name["one_sample"]] == 0 and got["n_points"][name["missing"]] == 0 and 0 < got["n_points"][name["few"]] < 100
    assert np.isnan(got["rms_after"][name["nan"]]) and np.isnan(got["rms_after"][name["missing"]]) and got["iterations"][name["nan"]] == 0
    # iterations = 1 and P = 1: one step of 20 mm is no convergence, the limit is reached
    one = _np(dr.refine_poses_depth(models, [3], P[:1, :3, :3], P[:1, :3, 3], K, depth[:1], **dict(params, iterations=1), debug=True))
    assert one["status"].tolist() == [1] and one["iterations"].tolist() == [1] and abs(one["t"][0, 2] - 520.0) < 1e-3 and one["trajectory"].shape == (1, 2, 4, 4)
    assert np.array_equal(_bits(one["trajectory"][0, 0]), _bits(P[0])) and np.array_equal(_bits(one["trajectory"][0, 1][:3, 3]), _bits(one["t"][0]))


@gpu
def test_bit_identical_across_streams_order_batch_and_grouping():
    scene = do.mixed()[0]
    models = ev.ObjectModels(scene["objects"])
    n = len(scene["obj_ids"])
    base = _mixed_call(models)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = _mixed_call(models)
    side.synchronize()
    perm = np.random.default_rng(0).permutation(n)
    shuffled = _mixed_call(models, rows=perm)
    grouped = _mixed_call(models, workspace_bytes=60000)
    assert base["n_groups"] == 1 and grouped["n_groups"] > 2
    for k in OUT:
        assert np.array_equal(_bits(base[k]), _bits(other[k])), k
        assert np.array_equal(_bits(base[k][perm]), _bits(shuffled[k])), k
        assert np.array_equal(_bits(base[k]), _bits(grouped[k])), k
    for p in (1, 4):
        alone = _mixed_call(models, rows=[p])
        for k in OUT:
            assert np.array_equal(_bits(base[k][p:p + 1]), _bits(alone[k])), (p, k)
    assert set(base["status"].tolist()) >= {1, 2, 3} and (base["iterations"] > 1).any()


@gpu
def test_refine_predictions_results_rows_and_vsd_recall():
    """refine_predictions equals direct refine_poses_depth calls; the "depth" rows parse back; on the convergence scene the refined rows
    score an AR_VSD no lower than the unrefined ones."""
    sc = do.convergence_scene()
    models = ev.ObjectModels(sc["objects"])
    direct = _conv_call(models)
    lines = {"stage_3": [], "depth": []}
    gt, cams, frames = {1: {}}, {1: {}}, {1: {}}
    targets = []
    for im in (0, 1):
        rows = np.where(sc["image_index"] == im)[0]
        far = [vo.pose(sc["start"][p][:3, :3], sc["start"][p][:3, 3] + F([0, 0, 300.0])) for p in rows]      # a second, hopeless hypothesis
        preds = [[{"R_stage_3": P[:3, :3].reshape(9), "t_stage_3": P[:3, 3].copy(), "inliers_ratio": q} for P, q in ((sc["start"][p], 0.9), (far[j], 0.5))]
                 for j, p in enumerate(rows)]
        ids = sc["obj_ids"][rows].tolist()
        out = pipeline.refine_predictions(preds, models, ids, sc["K"][im], sc["depth_mm"][im], **do.CONV_PARAMS)
        every = pipeline.refine_predictions(preds, models, ids, sc["K"][im], sc["depth_mm"][im], hypotheses="all", rank_by="depth", **do.CONV_PARAMS)
        for j, p in enumerate(rows):
            assert np.array_equal(_bits(out[j][0]["R_depth"]), _bits(direct["R"][p].reshape(9))) and np.array_equal(_bits(out[j][0]["t_depth"]), _bits(direct["t"][p]))
            assert out[j][0]["depth_status"] == direct["status"][p] and out[j][0]["depth_rms"] == float(direct["rms_after"][p]) and "R_depth" not in out[j][1]
            assert every[j][0]["inliers_ratio"] == 0.9 and every[j][1]["depth_status"] >= 2 and np.array_equal(_bits(every[j][0]["t_depth"]), _bits(direct["t"][p]))
        for stage in lines:
            lines[stage] += pipeline.bop_csv_lines(1, im, ids, [1.0] * len(ids), out, 0.1, stage=stage)
        gt[1][im] = {"obj_id": sc["obj_ids"][rows].astype(np.int64), "R": sc["gt"][rows][:, :3, :3].astype(np.float64), "t": sc["gt"][rows][:, :3, 3].astype(np.float64)}
        cams[1][im] = {"K": sc["K"][im].astype(np.float64), "depth_scale": 1.0}
        frames[1][im] = sc["depth_mm"][im]
        targets += [[1, im, int(o), 1] for o in ids]
    parsed = ev.read_bop_results(lines["depth"])
    assert np.array_equal(parsed["t"].astype(F), direct["t"]) and np.array_equal(parsed["R"].astype(F), direct["R"]) and parsed["im_id"].tolist() == [0, 0, 1, 1]
    score = {s: ev.match_and_score(ev.read_bop_results(lines[s]), gt, np.array(targets), models, cams, image_width=vo.W, depth_images=frames)
             for s in lines}
    print({s: (round(v["AR_VSD"], 4), round(v["AR_MSSD"], 4)) for s, v in score.items()})
    assert score["depth"]["AR_VSD"] >= score["stage_3"]["AR_VSD"] and score["depth"]["AR_MSSD"] >= score["stage_3"]["AR_MSSD"]
