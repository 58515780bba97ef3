"""CPU: what the RGB-D pose recovery (picopose_amd/rgbd_pose.py, pp_rgbd_ransac, its wiring in picopose_amd/pipeline.py) promises
without a device: the numpy restatement recovers planted poses, every problem the GPU tests use passes the margin check, the C
entry and the Python entries reject malformed arguments before any device work, and the results rows / the ICP start accept the
new stage."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rgbd_pose_oracle as ro  # noqa: E402
import test_rgbd_pose_gpu as gpu_tests  # noqa: E402  (the batch and the seeds the GPU tests use)

from picopose_amd import pipeline  # noqa: E402
from picopose_amd import rgbd_pose as rp  # noqa: E402  (absent before the feature)


def _pose_error(r, p):
    return np.abs(r["rot"] - p["R"]).max(), np.abs(r["tvec"] - p["t"]).max()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_recovers_planted_poses(seed):
    """Noise-free, no outliers: |dR| < 1e-5 and |dt| < 1e-5 max(|t|, 1) — the float32 rounding of the source points (6e-8 relative)
    times a conditioning of a few tens.  60 % outliers, 150 iterations: success on the planted inliers."""
    scene = ro.Scene(np.random.default_rng(seed))
    for prob, n in enumerate((64, 500, 3500)):
        p = ro.make_problem(scene, n, image=prob % 2)
        r = ro.solve(p, scene.depth, prob)
        dR, dt = _pose_error(r, p)
        assert r["ok"] and r["ratio"] == 1.0 and r["npts"] == r["nlisted"] == n and r["mask"].sum() == n
        assert dR < 1e-5 and dt < 1e-5 * max(np.linalg.norm(p["t"]), 1.0), (n, dR, dt)
    p = ro.make_problem(scene, 3500, outlier_frac=0.6, noise=0.001, image=1)
    r = ro.solve(p, scene.depth, 3, 150)
    dR, dt = _pose_error(r, p)
    assert r["ok"] and 0.3 < r["ratio"] <= 0.4 + 0.02 and dR < 2e-3 and dt < 5e-4, (r["ratio"], dR, dt)
    assert r["rms"] < 0.005 and int(r["mask"].sum()) == round(r["ratio"] * r["npts"])


def test_oracle_follows_the_gather_and_failure_clauses():
    problems, depth = gpu_tests.batch()
    want = gpu_tests.expected(150)
    for w, (n, kw) in zip(want, gpu_tests.CASES):
        assert w["nlisted"] == n
        if not w["ok"]:
            assert np.array_equal(w["rot"], np.eye(3)) and w["tvec"].tolist() == [0.0, 0.0, 1.0] and w["ratio"] == 0.0 and w["rms"] == 0.0
            assert not w["mask"].any()
    assert [w["npts"] for w in want] == [3500, 0, 2, 3, 4, 64, 65, 513, 4096, 3500, 180, 0, 200, 100, 0, 850]
    assert [w["ok"] for w in want] == [True, False, False, True, True, True, True, True, True, True, True, False, False, False, False, True]
    # a dropped entry never shows in the mask; the listed order is the list's
    p, w = problems[15], want[15]
    ps, pq, lidx, nl = ro.gather(p, depth)
    assert nl == 1000 and len(lidx) == 850 and np.all(np.diff(lidx) > 0) and not w["mask"][np.setdiff1d(np.arange(ro.MAXP), lidx)].any()
    assert ps.dtype == np.float32 and pq.dtype == np.float32
    # the draws: three distinct indices, a function of (problem, hypothesis) alone
    assert ro.draw(0, 0, 3500) == ro.draw(0, 0, 3500) != ro.draw(1, 0, 3500) and sorted(ro.draw(4, 9, 3)) == [0, 1, 2]
    assert ro.mix(0) == 0 and 0 < ro.mix(1) < 2 ** 32          # (the finaliser maps 0 to 0)


@pytest.mark.parametrize("iterations", gpu_tests.ITERATIONS)
def test_every_gpu_problem_passes_the_margin_check(iterations):
    """No residual within 1e-7 inlier_dist of inlier_dist, no degeneracy decision within a relative 1e-3 of its bound: the consensus
    sets the GPU tests compare bit for bit do not depend on rounding.  A seed that fails here is replaced, never skipped."""
    for i, w in enumerate(gpu_tests.expected(iterations)):
        assert ro.margins(w), (i, w["margin_dist"], w["margin_deg"])


def test_c_entry_rejects_malformed_arguments_before_any_launch():
    from picopose_amd import _lib

    L = _lib.lib()
    assert "pp_rgbd_ransac" in _lib.declared_symbols()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    # tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, P, H, W, N, depth, n_images, dH, dW, image_index, inlier_dist, iterations,
    # rot, tvec, inlier_ratio, success, num_points, num_listed, rms, inlier_mask, stream
    good = [p] * 6 + [2, 64, 64, 4096, p, 2, 120, 160, p, p, 150] + [p] * 7 + [None, None]
    pointers = [0, 1, 2, 3, 4, 5, 10, 14, 15, 17, 18, 19, 20, 21, 22, 23]          # every pointer but inlier_mask (24) and the stream
    for k in pointers:
        bad = list(good)
        bad[k] = None
        assert L.pp_rgbd_ransac(*bad) == -1, k
    for k, v in ((6, 0), (6, -1), (7, 0), (8, 0), (9, 0), (9, 4097), (11, 0), (11, -3), (12, 0), (13, 0), (13, -1), (16, 0), (16, -5)):
        bad = list(good)
        bad[k] = v
        assert L.pp_rgbd_ransac(*bad) == -1, (k, v)


def _args(P=2, N=16, H=8, W=8):
    z = torch.zeros
    return [z(P, 2, H, W), z(P, 3, H, W), z(P, 3, 3), z(P, 4, 4), z(P, N, 2, dtype=torch.int64), z(P, N, 2, dtype=torch.int64)]


def test_python_entries_reject_malformed_arguments_before_any_device_work():
    """CPU tensors throughout: a call that got past validation would raise PicoPoseHipError (inputs must be on the GPU), not ValueError."""
    depth = torch.ones(2, 12, 16)
    entries = (rp.pose_recovery_ransac_rgbd_batched, rp.pose_recovery_ransac_rgbd_batched_async, rp.rgbd_launch)

    def rejected(args, depth_, dist, **kw):
        for f in entries:
            with pytest.raises(ValueError):
                f(*args, depth_, dist, **kw)

    for k, shape in ((0, (2, 3, 8, 8)), (0, (2, 2, 8)), (1, (2, 3, 8, 9)), (1, (3, 3, 8, 8)), (2, (3, 3)), (2, (1, 3, 3)), (3, (2, 3, 4)),
                     (4, (2, 16, 3)), (4, (2, 17, 2)), (5, (1, 16, 2)), (4, (2, 5000, 2))):
        bad = _args()
        bad[k] = torch.zeros(shape, dtype=bad[k].dtype)
        if k == 4 and shape == (2, 5000, 2):
            bad[5] = torch.zeros(shape, dtype=bad[5].dtype)
        rejected(bad, depth, 0.01)
    rejected(_args(), depth, None)                                       # inlier_dist has no default
    rejected(_args(), depth, torch.ones(3))
    rejected(_args(), depth, "5 mm")
    rejected(_args(), torch.ones(16), 0.01)                              # depth neither 2-D nor 3-D
    rejected(_args(), torch.ones(1, 2, 12, 16), 0.01)
    rejected(_args(), torch.ones(2, 12, 16, dtype=torch.int32), 0.01)
    rejected(_args(), np.ones((2, 12, 16), np.uint16), 0.01)             # raw depth without its scale
    rejected(_args(), np.ones((2, 12, 16), np.uint16), 0.01, depth_scale=-1.0)
    rejected(_args(), depth, 0.01, depth_scale=0.1)                      # float depth with a raw scale
    rejected(_args(), depth, 0.01, depth_unit="cm")
    rejected(_args(), depth, 0.01, image_index=torch.zeros(3, dtype=torch.int32))
    rejected(_args(), depth, 0.01, iterations=0)
    rejected(_args(), depth, 0.01, iterations=1.5)
    with pytest.raises(TypeError):
        rp.pose_recovery_ransac_rgbd_batched(*_args(), depth)            # (a required positional argument)
    one = [a[0] for a in _args()]
    for bad_depth in (depth, torch.ones(16)):
        with pytest.raises(ValueError):
            rp.pose_recovery_ransac_rgbd(*one, bad_depth, 0.01)          # one problem reads one image
    with pytest.raises(ValueError):
        rp.pose_recovery_ransac_rgbd(*one, depth[0], None)
    with pytest.raises(ValueError):
        rp.pose_recovery_ransac_rgbd(*_args(), depth[0], 0.01)
    # well-formed arguments get past validation and stop at the device check
    from picopose_amd._lib import PicoPoseHipError
    with pytest.raises(PicoPoseHipError):
        rp.pose_recovery_ransac_rgbd_batched(*_args(), depth, 0.01, torch.zeros(2, dtype=torch.int32))
    assert rp.check_rgbd_args(*_args(), depth[0], [0.01, 0.02]) == (2, 8, 8, 16, 1, 12, 16)
    doc = rp.pose_recovery_ransac_rgbd_batched.__doc__
    assert "unit of src_pts_3d" in doc and "diameter" in doc and "no default" in doc


def test_pipeline_depth_arguments_are_checked_before_the_forward():
    class Net:
        def __call__(self, *a, **k):
            raise AssertionError("the forward ran")

    depth = np.ones((12, 16), np.float32)
    for kw in (dict(depth=depth), dict(rgbd_inlier_dist=0.01), dict(depth_scale=0.1), dict(depth=np.ones((2, 12, 16), np.float32), rgbd_inlier_dist=0.01),
               dict(depth=np.ones(16, np.float32), rgbd_inlier_dist=0.01)):
        with pytest.raises(ValueError):
            pipeline.infer_batch(Net(), {}, **kw)
        with pytest.raises(ValueError):
            pipeline.infer_image(Net(), {"score": torch.zeros(1, 2)}, {}, **kw)


def _preds(rgbd=True):
    def hyp(r, z):
        h = {"R_stage_3": np.eye(3).reshape(9), "t_stage_3": np.array([0.0, 0.0, z]), "inliers_ratio": r}
        if rgbd:
            h.update(R_rgbd=np.eye(3)[::-1].reshape(9).copy(), t_rgbd=np.array([1.0, 2.0, z + 7.0]), rgbd_inliers_ratio=0.5, rgbd_success=True)
        return h
    return [[hyp(0.9, 400.0), hyp(0.8, 410.0)], [hyp(0.6, 430.0)]]


def test_results_rows_of_the_rgbd_stage():
    from picopose_amd import evaluation as ev

    assert pipeline.STAGES["rgbd"] == ("R_rgbd", "t_rgbd")
    preds = _preds()
    rows = ev.read_bop_results(pipeline.bop_csv_lines(3, 7, [1, 2], [0.5, 0.25], preds, 1.5, stage="rgbd"))
    assert rows["t"].tolist() == [[1.0, 2.0, 407.0], [1.0, 2.0, 437.0]] and rows["obj_id"].tolist() == [1, 2]
    assert np.array_equal(rows["R"][0], np.eye(3)[::-1])
    assert pipeline.bop_csv_lines(3, 7, [1, 2], [0.5, 0.25], preds, 1.5) == pipeline.bop_csv_lines(3, 7, [1, 2], [0.5, 0.25], _preds(False), 1.5)
    with pytest.raises(ValueError):
        pipeline.bop_csv_lines(3, 7, [1, 2], [0.5, 0.25], _preds(False), 1.5, stage="rgbd")       # no depth image was given
    with pytest.raises(ValueError):
        pipeline.bop_csv_lines(3, 7, [1, 2], [0.5, 0.25], preds, 1.5, stage="rgb-d")


def test_refine_predictions_start_argument(monkeypatch):
    from picopose_amd import depth_refine as dr

    calls = []

    def fake(models, ids, R, t, K_, depth, depth_scale=None, **kw):
        calls.append((np.asarray(R).copy(), np.asarray(t).copy(), kw))
        n = len(ids)
        return {"R": torch.eye(3).repeat(n, 1, 1), "t": torch.zeros(n, 3), "status": torch.zeros(n, dtype=torch.int32),
                "rms_after": torch.ones(n, dtype=torch.float32)}

    monkeypatch.setattr(dr, "refine_poses_depth", fake)
    K, d = np.eye(3), np.zeros((12, 16), np.float32)
    preds = _preds()
    out = pipeline.refine_predictions(preds, None, [1, 2], K, d)
    assert calls[-1][1][:, 2].tolist() == [400.0, 430.0] and np.array_equal(calls[-1][0][0], np.eye(3)) and calls[-1][2] == {}
    same = pipeline.refine_predictions(preds, None, [1, 2], K, d, start="stage_3")
    assert np.array_equal(calls[-1][1], calls[-2][1]) and same[0][0].keys() == out[0][0].keys()
    chained = pipeline.refine_predictions(preds, None, [1, 2], K, d, start="rgbd", hypotheses="all", iterations=3)
    assert calls[-1][1].tolist() == [[1.0, 2.0, 407.0], [1.0, 2.0, 417.0], [1.0, 2.0, 437.0]] and np.array_equal(calls[-1][0][1], np.eye(3)[::-1])
    assert calls[-1][2] == {"iterations": 3}                               # `start` is not passed on
    assert chained[0][1]["depth_status"] == 0 and "R_depth" not in preds[0][0]
    n = len(calls)
    for kw in (dict(start="depth"), dict(start=None), dict(start="RGBD"), dict(start=["rgbd"])):
        with pytest.raises(ValueError):
            pipeline.refine_predictions(preds, None, [1, 2], K, d, **kw)
    with pytest.raises(ValueError):
        pipeline.refine_predictions(_preds(False), None, [1, 2], K, d, start="rgbd")      # no RGB-D pose to start from
    assert len(calls) == n
