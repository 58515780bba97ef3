"""GPU: the batched 3D-3D RANSAC on the test depth image (pp_rgbd_ransac; picopose_amd/rgbd_pose.py and its wiring in
picopose_amd/pipeline.py) against the numpy restatement of tests/rgbd_pose_oracle.py.

The problems are fixed by SCENE_SEED below; tests/test_rgbd_pose_cpu.py asserts, without a GPU, that every one of them passes the
oracle's margin check (no inlier or degeneracy decision within rounding of its bound), so the consensus sets are fixed by the
contract and the masks must be bit-equal.  The 1e-9 bars on R, t and rms are derived, not measured: both sides work in float64 on
the same float32 pairs, the consensus sets are well spread (eigen-gap of order one), so a converged Jacobi vector and an SVD agree
to about 1e-13; 1e-9 leaves four orders of margin."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rgbd_pose_oracle as ro  # noqa: E402

gpu = pytest.mark.gpu
KEYS = ("tar2d", "src3d", "K", "pose", "tar_pts", "src_pts")
SCENE_SEED = 7
ITERATIONS = (150, 1, 256)
# (n_listed, keywords of rgbd_pose_oracle.make_problem): listed counts 0, 2, 3, 4, 64, 65, 513, 3500, 4096 across the wave (64), the
# workgroup (512) and the LDS-capacity (4096) edges; 0 / 30 / 60 % outliers; two depth images in mixed order
CASES = (
    (3500, dict(outlier_frac=0.6, noise=0.001, image=0)),
    (0, dict(image=1)),
    (2, dict(image=0)),
    (3, dict(image=0)),
    (4, dict(image=1)),
    (64, dict(image=1)),
    (65, dict(outlier_frac=0.3, image=0)),
    (513, dict(outlier_frac=0.3, noise=0.0005, image=1)),
    (4096, dict(outlier_frac=0.3, image=0)),
    (3500, dict(noise=0.001, image=1)),
    (300, dict(n_missing=120, image=0)),                     # its only failures are missing depth
    (100, dict(n_outside=100, image=1)),                     # every entry outside the image
    (200, dict(collinear=True, image=0)),                    # all source points on one line: a failure
    (100, dict(inlier_dist=0.0, image=1)),                   # inlier_dist = 0: a failure
    (100, dict(image=0)),                                    # image_index out of range (set below): a failure, nothing read
    (1000, dict(outlier_frac=0.3, noise=0.001, n_missing=100, n_outside=50, image=1)),
)
BAD_IMAGE = 14


@functools.lru_cache(maxsize=None)
def batch():
    """-> (problems, depth (2, 120, 160) float32): the one batch every test here shares."""
    scene = ro.Scene(np.random.default_rng(SCENE_SEED))
    problems = [ro.make_problem(scene, n, **kw) for n, kw in CASES]
    problems[BAD_IMAGE]["image"] = 5
    return problems, scene.depth


@functools.lru_cache(maxsize=None)
def expected(iterations=150):
    problems, depth = batch()
    return [ro.solve(p, depth, i, iterations) for i, p in enumerate(problems)]


def _dev(problems):
    return [torch.from_numpy(np.stack([p[k] for p in problems])).cuda() for k in KEYS]


def _extra(problems):
    return (np.array([p["inlier_dist"] for p in problems], np.float32), np.array([p["image"] for p in problems], np.int32))


@functools.lru_cache(maxsize=None)
def launched(iterations=150):
    from picopose_amd.rgbd_pose import pose_recovery_ransac_rgbd_batched

    problems, depth = batch()
    dist, img = _extra(problems)
    return pose_recovery_ransac_rgbd_batched(*_dev(problems), torch.from_numpy(depth).cuda(), dist, img, iterations, return_inliers=True)


def _against_oracle(got, want, problems):
    rot, tvec, ratio, ok, npts, st, mask = got
    for i, (w, p) in enumerate(zip(want, problems)):
        assert bool(ok[i]) == w["ok"] and npts[i] == w["npts"] and st["num_listed"][i] == w["nlisted"], (i, ok[i], npts[i], st["num_listed"][i])
        assert np.array_equal(mask[i], w["mask"]), (i, int(mask[i].sum()), int(w["mask"].sum()))
        assert ratio[i] == w["ratio"], (i, ratio[i], w["ratio"])
        dR, dt = np.abs(rot[i] - w["rot"]).max(), np.abs(tvec[i, :, 0] - w["tvec"]).max()
        drms = abs(st["rms"][i] - w["rms"])
        print(f"problem {i}: ok {w['ok']} npts {w['npts']} ratio {w['ratio']:.4f} dR {dR:.3g} dt {dt:.3g} drms {drms:.3g}")
        assert dR <= 1e-9 and dt <= 1e-9 * max(np.linalg.norm(w["tvec"]), 1.0), (i, dR, dt)
        assert drms <= 1e-9 * max(w["rms"], float(p["inlier_dist"])), (i, st["rms"][i], w["rms"])
        if not w["ok"]:      # the failure outputs, bit for bit
            assert np.array_equal(rot[i], np.eye(3)) and np.array_equal(tvec[i, :, 0], [0.0, 0.0, 1.0]) and st["rms"][i] == 0.0


@gpu
def test_batch_equals_the_oracle():
    problems, _ = batch()
    want = expected(150)
    _against_oracle(launched(150), want, problems)
    ok = [w["ok"] for w in want]
    assert ok == [True, False, False, True, True, True, True, True, True, True, True, False, False, False, False, True]
    assert want[10]["npts"] == 180 and want[11]["npts"] == 0 and want[12]["npts"] == 200 and want[BAD_IMAGE]["npts"] == 0
    for i in (0, 7, 8, 9, 15):       # the planted pose is found (noise 0 - 1 mm, up to 60 % outliers)
        assert np.abs(launched(150)[0][i] - problems[i]["R"]).max() < 2e-3 and np.abs(launched(150)[1][i, :, 0] - problems[i]["t"]).max() < 5e-4


@gpu
@pytest.mark.parametrize("iterations", [1, 256])
def test_other_iteration_counts_equal_the_oracle(iterations):
    _against_oracle(launched(iterations), expected(iterations), batch()[0])


def _same(a, b):
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x)
        else:
            assert np.array_equal(x, y)


@gpu
def test_launches_are_deterministic_and_capped_at_256_hypotheses():
    from picopose_amd.rgbd_pose import pose_recovery_ransac_rgbd_batched

    problems, depth = batch()
    dist, img = _extra(problems)
    run = lambda it: pose_recovery_ransac_rgbd_batched(*_dev(problems), torch.from_numpy(depth).cuda(), dist, img, it, True)  # noqa: E731
    _same(run(150), launched(150))
    _same(run(300), launched(256))


@gpu
def test_single_problem_wrapper_and_async_handle():
    from picopose_amd.rgbd_pose import pose_recovery_ransac_rgbd, pose_recovery_ransac_rgbd_batched_async

    problems, depth = batch()
    dist, img = _extra(problems)
    base = launched(150)
    p = problems[0]
    assert p["image"] == 0
    r, tv, ra, ok, n, st, m = pose_recovery_ransac_rgbd(*[torch.from_numpy(p[k]).cuda() for k in KEYS], torch.from_numpy(depth[0]).cuda(),
                                                        float(p["inlier_dist"]), return_inliers=True)
    assert ok and ra == base[2][0] and n == base[4][0] and np.array_equal(r, base[0][0]) and np.array_equal(tv, base[1][0])
    assert st == dict(num_listed=base[5]["num_listed"][0], rms=base[5]["rms"][0]) and np.array_equal(m, base[6][0])
    side = torch.cuda.Stream()
    h = pose_recovery_ransac_rgbd_batched_async(*_dev(problems), torch.from_numpy(depth).cuda(), torch.from_numpy(dist).cuda(),
                                                torch.from_numpy(img).cuda(), 150, True, stream=side)
    _same(h.result(), base)
    # raw uint16 depth with its scale and float millimetres are converted on the device: 0.1 mm steps of 8000..10000 units
    u16 = np.clip(np.round(depth * 10000.0), 0, 65535).astype(np.uint16)
    metres = ((u16.astype(np.float32) * np.float32(0.1)) / np.float32(1000.0)).astype(np.float32)
    from picopose_amd.rgbd_pose import depth_on_device
    assert np.array_equal(depth_on_device(u16, torch.device("cuda"), 0.1).cpu().numpy(), metres)
    assert np.array_equal(depth_on_device(depth * np.float32(1000.0), torch.device("cuda"), None, "mm").cpu().numpy(),
                          (torch.from_numpy(depth * np.float32(1000.0)) * 1e-3).numpy())


@gpu
def test_rgbd_for_outputs_equals_the_direct_call_reshaped():
    from picopose_amd.pipeline import rgbd_collect, rgbd_for_outputs, rgbd_for_outputs_async
    from picopose_amd.rgbd_pose import pose_recovery_ransac_rgbd_batched

    problems, depth = batch()
    hyp, B = 2, 3
    pick = [[0, 5, 7], [8, 9, 15]]                          # outputs[k] holds instance b's problem pick[k][b]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    stack = lambda k, key: cuda(np.stack([problems[i][key] for i in pick[k]]))  # noqa: E731
    outputs = [dict(tar_pts_2d=stack(k, "tar2d"), src_pts_3d=stack(k, "src3d"), tem_pose=stack(k, "pose"), pred_tar_pts=stack(k, "tar_pts"),
                    pred_src_pts=stack(k, "src_pts"), pred_poses=torch.eye(4).repeat(B, 1, 1).cuda()) for k in range(hyp)]
    real_K = cuda(np.stack([ro.K0] * B))
    img_b = np.array([0, 1, 1], np.int32)                   # (both hypotheses of an instance read the instance's image)
    assert all(problems[pick[k][b]]["image"] == img_b[b] for k in range(hyp) for b in range(B))
    dist_b = np.array([0.005, 0.004, 0.006], np.float32)
    flat = [problems[i] for k in range(hyp) for i in pick[k]]
    direct = pose_recovery_ransac_rgbd_batched(*_dev(flat), cuda(depth), np.tile(dist_b, hyp), np.tile(img_b, hyp), return_inliers=True)
    got = rgbd_for_outputs(outputs, real_K, cuda(depth), dist_b, img_b, return_inliers=True)
    assert got[0].shape == (hyp, B, 3, 3) and got[1].shape == (hyp, B, 3, 1) and got[3].shape == (hyp, B) and got[6].shape == (hyp, B, ro.MAXP)
    assert got[3].all()
    for g, d in zip(got, direct):
        if isinstance(g, dict):
            assert all(np.array_equal(g[k].reshape(-1), d[k]) for k in d)
        else:
            assert np.array_equal(g.reshape(d.shape), d)
    side = torch.cuda.Stream()
    _same(rgbd_collect(rgbd_for_outputs_async(outputs, real_K, cuda(depth), dist_b, img_b, return_inliers=True, stream=side), hyp, B), got)


@gpu
def test_infer_batch_and_infer_image_carry_the_rgbd_pose(monkeypatch):
    """The smallest network, random weights, a random positive depth: every hypothesis carries the four new keys, they equal
    rgbd_for_outputs on the same forward, and the result without depth is what it was (the keys added, nothing else moved)."""
    from netcfg import make_end_points, small_cfg

    from picopose_amd import ops
    from picopose_amd.picopose import Net
    from picopose_amd.pipeline import infer_batch, infer_image, rgbd_for_outputs
    from picopose_amd.utils.seeding import seeded_state_dict

    # (plain seeded weights leave the f16x3 operand range, as in test_e2e.py::test_infer_image_walks_instances_like_run_test: the
    # sticky saturation word would, rightly, refuse these poses.  This test is about the wiring, not the numbers: reporting off.)
    monkeypatch.setattr(ops, "SATURATION_FLAG", False)
    B, N, hyp = 2, 4, 2
    net = Net(small_cfg())
    net.load_state_dict(seeded_state_dict(net.state_dict(), 21))
    net = net.cuda().eval()
    ep = {k: v.cuda() for k, v in make_end_points(B, N, 33, dome=True).items()}
    depth = (0.5 + torch.rand(480, 640, generator=torch.Generator().manual_seed(3))).cuda()
    dist = 0.05
    with torch.no_grad():
        ep["template_feature"] = torch.stack([net.feature_extractor(ep["tem_rgb"][b])[-1] for b in range(B)])
        plain = infer_batch(net, ep, hyp)
        with_depth = infer_batch(net, ep, hyp, depth=depth, rgbd_inlier_dist=dist)
        outputs = net(ep, hyp)
    rot, tvec, ratio, ok, npts, st = rgbd_for_outputs(outputs, ep["real_K"], depth, dist)
    assert (npts <= st["num_listed"]).all()
    print("listed", st["num_listed"].tolist(), "with a depth", npts.tolist(), "rgbd success", ok.tolist())
    stage3_ratio = lambda h: h["inliers_ratio"]  # noqa: E731
    for b in range(B):
        assert len(plain[b]) == len(with_depth[b]) == hyp
        for a, w in zip(plain[b], with_depth[b]):
            assert set(w) == set(a) | {"R_rgbd", "t_rgbd", "rgbd_inliers_ratio", "rgbd_success"}
            for k in a:       # without the new keys: bit-equal to the result without depth
                assert np.array_equal(np.asarray(a[k]), np.asarray(w[k])), k
        assert [stage3_ratio(h) for h in plain[b]] == [stage3_ratio(h) for h in with_depth[b]]
        # each hypothesis k of the forward is found among the instance's dicts by its RGB-D ratio and pose
        for k in range(hyp):
            want_R = rot[k, b].reshape(9) if ok[k, b] else None
            match = [w for w in with_depth[b] if w["rgbd_inliers_ratio"] == float(ratio[k, b]) and w["rgbd_success"] == bool(ok[k, b])
                     and (want_R is None or np.array_equal(w["R_rgbd"], want_R))]
            assert match, (b, k)
            w = match[0]
            if ok[k, b]:
                assert np.array_equal(w["t_rgbd"], tvec[k, b, :, 0])
            else:
                assert np.array_equal(w["R_rgbd"], np.asarray(w["R"]).reshape(9)) and np.array_equal(w["t_rgbd"], np.asarray(w["t"]).reshape(3))
    with pytest.raises(ValueError):
        infer_batch(net, ep, hyp, depth=depth)
    # infer_image: both walks give the same rows; one mini-batch of both instances is infer_batch's forward, t_rgbd in millimetres
    data = {k: v[None] for k, v in ep.items() if k.startswith("real_")}
    data["obj_idx"] = torch.tensor([[0, 1]], device="cuda")
    data["score"] = torch.tensor([[0.9, 0.8]], device="cuda")
    tem = {k: v for k, v in ep.items() if k.startswith("tem_") or k == "template_feature"}
    with torch.no_grad():
        rows = [infer_image(net, data, tem, hyp=hyp, bs=1, pipelined=pl, depth=depth, rgbd_inlier_dist=[dist, dist]) for pl in (True, False)]
        whole = infer_image(net, data, tem, hyp=hyp, bs=2, depth=depth.cpu().numpy(), rgbd_inlier_dist=dist)
    for inst_p, inst_s, inst_w, inst_b in zip(rows[0], rows[1], whole, with_depth):
        for hp, hs, hw, hb in zip(inst_p, inst_s, inst_w, inst_b):
            assert set(hp) == {"R_stage_3", "t_stage_3", "inliers_ratio", "R_rgbd", "t_rgbd", "rgbd_inliers_ratio", "rgbd_success"}
            assert all(np.array_equal(np.asarray(hp[k]), np.asarray(hs[k])) for k in hp)
            assert np.array_equal(hw["t_stage_3"], np.asarray(hb["t"]).reshape(3) * 1000) and hw["inliers_ratio"] == hb["inliers_ratio"]
            assert np.array_equal(hw["t_rgbd"], hb["t_rgbd"] * 1000) and np.array_equal(hw["R_rgbd"], hb["R_rgbd"])
            assert hw["rgbd_inliers_ratio"] == hb["rgbd_inliers_ratio"] and hw["rgbd_success"] == hb["rgbd_success"]
    with pytest.raises(ValueError):
        infer_image(net, data, tem, hyp=hyp, depth=depth)


@gpu
def test_refine_predictions_starts_from_the_rgbd_pose():
    """One planted problem on the depth-refinement convergence scene: pairs of a pixel and the object-frame point its measured depth
    back-projects to under the ground truth; the RGB-D pose (millimetres throughout) is the start of the ICP, which ends with
    depth_status <= 1."""
    import depth_refine_oracle as do

    from picopose_amd import evaluation as ev
    from picopose_amd import pipeline
    from picopose_amd.rgbd_pose import pose_recovery_ransac_rgbd

    sc = do.convergence_scene()
    p, im = 0, int(sc["image_index"][0])
    K, depth = sc["K"][im].astype(np.float32), sc["depth_mm"][im].astype(np.float32)
    Pg = sc["gt"][p].astype(np.float64)
    rng = np.random.default_rng(11)
    uvz = Pg[:3, 3] @ K.astype(np.float64).T
    cu, cv = uvz[0] / uvz[2], uvz[1] / uvz[2]
    yy, xx = np.nonzero((depth > 0) & (depth < 1400.0))       # off the wall
    near = np.flatnonzero((np.abs(xx - cu) < 25) & (np.abs(yy - cv) < 25))
    sel = rng.permutation(near)[:400]
    assert len(sel) >= 100
    u, v, z = xx[sel].astype(np.float32), yy[sel].astype(np.float32), depth[yy[sel], xx[sel]].astype(np.float64)
    K64 = K.astype(np.float64)
    q = np.stack([(u - K64[0, 2]) * z / K64[0, 0], (v - K64[1, 2]) * z / K64[1, 1], z], axis=1)
    src = (q - Pg[:3, 3]) @ Pg[:3, :3]
    maps = ro.pack(rng, u, v, src)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    R, t, ratio, ok, n, st = pose_recovery_ransac_rgbd(cuda(maps["tar2d"]), cuda(maps["src3d"]), cuda(K), torch.eye(4).cuda(),
                                                       cuda(maps["tar_pts"]), cuda(maps["src_pts"]), cuda(depth), 1.0)
    assert ok and n == len(sel) and ratio == 1.0
    assert np.abs(R - Pg[:3, :3]).max() < 1e-4 and np.abs(t[:, 0] - Pg[:3, 3]).max() < 0.05      # (float32 source points, millimetres)
    far = sc["start"][p]
    preds = [[{"R_stage_3": far[:3, :3].reshape(9), "t_stage_3": far[:3, 3] + np.float32([0, 0, 300.0]), "inliers_ratio": 0.9,
               "R_rgbd": R.reshape(9), "t_rgbd": t[:, 0], "rgbd_inliers_ratio": ratio, "rgbd_success": True}]]
    models = ev.ObjectModels(sc["objects"])
    out = pipeline.refine_predictions(preds, models, [int(sc["obj_ids"][p])], sc["K"][im], sc["depth_mm"][im], start="rgbd", **do.CONV_PARAMS)
    assert out[0][0]["depth_status"] <= 1, out[0][0]["depth_status"]
    hopeless = pipeline.refine_predictions(preds, models, [int(sc["obj_ids"][p])], sc["K"][im], sc["depth_mm"][im], **do.CONV_PARAMS)
    assert hopeless[0][0]["depth_status"] >= 2                 # (the stage_3 start, 300 mm off, is what the default still refines)
    assert pipeline.bop_csv_lines(1, im, [int(sc["obj_ids"][p])], [1.0], out, 0.1, stage="rgbd")[0].startswith(f"1,{im},")
