"""GPU: the Levenberg-Marquardt pose refinement of the batched PnP (refine="lm", pp_pnp_ransac_refine) and its standalone form
(solve_pnp_refine_lm, pp_pnp_refine_lm), against ground truth, against the numpy oracle of tests/pnp_refine_oracle.py, and against
the unrefined launch it must not disturb."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pnp_refine_oracle as oref  # noqa: E402
from pnp_problems import make_batch, pose_errors  # noqa: E402

gpu = pytest.mark.gpu
KEYS = ("tar2d", "src3d", "K", "pose", "tar_pts", "src_pts")


def _problem(rng, n_pts, n_out=0, noise=0.0):
    b = make_batch(rng, 1, n_pts, (n_out / n_pts) if n_pts else 0.0, noise)
    return {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in b.items()}


def _dev(problems):
    return [torch.from_numpy(np.stack([p[k] for p in problems])).cuda() for k in KEYS]


def _batch_dev(b):
    return [torch.from_numpy(b[k]).cuda() for k in KEYS]


def _unbatch(b):
    return [{k: b[k][i] for k in KEYS} for i in range(b["tar2d"].shape[0])]


def _run(args, **kw):
    from picopose_amd.utils.pose_recovery import pose_recovery_ransac_pnp_batched

    return pose_recovery_ransac_pnp_batched(*args, return_npts=True, **kw)


@gpu
def test_refinement_leaves_the_consensus_untouched():
    from picopose_amd.utils.pose_recovery import pose_recovery_ransac_pnp

    rng = np.random.default_rng(20)
    probs = [_problem(rng, 300), _problem(rng, 3500, noise=0.5), _problem(rng, 2000, n_out=1200, noise=0.3),
             _problem(rng, 500, n_out=150, noise=1.0), _problem(rng, 4), _problem(rng, 0), _problem(rng, 3)]
    args = _dev(probs)
    rot0, tvec0, ratio0, ok0, npts0 = _run(args)
    rot1, tvec1, ratio1, ok1, npts1, st, mask = _run(args, refine="lm", return_inliers=True)
    assert np.array_equal(ratio0, ratio1) and np.array_equal(ok0, ok1) and np.array_equal(npts0, npts1)
    assert ok0[:4].all() and not ok0[4:].any()
    for i in range(len(probs)):
        assert int(mask[i].sum()) == round(ratio1[i] * npts1[i]) and not mask[i, npts1[i]:].any()
        if not ok1[i]:       # the reference's failure outputs, no refinement, an empty mask
            assert np.array_equal(rot1[i], np.eye(3)) and np.array_equal(tvec1[i], np.array([[0.0], [0.0], [1.0]])) and ratio1[i] == 0.0
            assert st["rms_before"][i] == 0.0 and st["rms_after"][i] == 0.0 and st["iterations"][i] == 0
        else:
            assert st["iterations"][i] > 0 and st["rms_after"][i] <= st["rms_before"][i]
    # pose_recovery_ransac_pnp: same answer, plus the stats and the mask (problem 0: a problem's sampling depends on its batch index)
    p = probs[0]
    r, tv, ra, ok, st1, m1 = pose_recovery_ransac_pnp(*[torch.from_numpy(p[k]).cuda() for k in KEYS], refine="lm", return_inliers=True)
    assert ok and ra == ratio1[0] and np.array_equal(r, rot1[0]) and np.array_equal(tv, tvec1[0]) and np.array_equal(m1, mask[0])
    assert st1 == dict(rms_before=st["rms_before"][0], rms_after=st["rms_after"][0], iterations=st["iterations"][0])


@gpu
@pytest.mark.parametrize("n", [8, 64, 3500])
def test_noise_free_problems_refine_to_the_planted_pose(n):
    """float32-exact correspondences (tests/pnp_refine_oracle.exact_problem): the planted pose is the minimum of the cost."""
    rng = np.random.default_rng(30 + n)
    made = [oref.exact_problem(rng, n) for _ in range(4)]
    rot, tvec, ratio, ok, npts, st = _run(_dev([m[0] for m in made]), refine="lm")
    for i, (_, R, t) in enumerate(made):
        assert ok[i] and ratio[i] == 1.0 and npts[i] == n
        assert np.abs(rot[i] - R).max() < 1e-9, (i, np.abs(rot[i] - R).max())
        assert np.abs(tvec[i, :, 0] - t).max() < 1e-9 * max(np.linalg.norm(t), 1.0)   # (|t| < 1 here: an absolute 1e-9)
        assert st["rms_after"][i] < 1e-6 and st["rms_after"][i] <= st["rms_before"][i]
    # float32-rounded random problems: the refined pose is the oracle's minimum on the same data, within ~1e-6 of the planted one.
    # (1e-7, not 1e-9: the kernel forms the object-frame points (X - t_tem) R_tem in float32 with fused multiply-adds, oracle.pnp.gather_valid
    # rounds every product, and the ~1e-9 m between the two point sets moves an 8-point minimum by up to ~1e-8)
    b = make_batch(rng, 3, n)
    rot, tvec, ratio, ok, npts, st = _run(_batch_dev(b), refine="lm")
    rot0, tvec0 = _run(_batch_dev(b))[:2]
    assert ok.all() and np.all(ratio == 1.0)
    for i, p in enumerate(_unbatch(b)):
        p3, p2 = oref.problem_points(p)
        Ro, to, co, _ = oref.refine_lm(p3, p2, oref.cam_of(p["K"]), rot0[i], tvec0[i])
        assert np.abs(rot[i] - Ro).max() < 1e-7 and np.abs(tvec[i, :, 0] - to).max() < 1e-7
        assert np.abs(rot[i] - b["R"][i]).max() < 2e-5 and st["rms_after"][i] < 1e-4


def _oracle_check(p, R0, t0, mask_row, R1, t1, rms1, tol=1e-7):
    p3, p2 = oref.problem_points(p)
    use = mask_row[:len(p3)]
    Ro, to, co, _ = oref.refine_lm(p3[use], p2[use], oref.cam_of(p["K"]), R0, t0)
    assert np.abs(R1 - Ro).max() < tol and np.abs(t1.reshape(3) - to).max() < tol, (np.abs(R1 - Ro).max(), np.abs(t1.reshape(3) - to).max())
    # the kernel's pose is the oracle's minimum: its cost on the oracle's data is not above the oracle's (the kernel's own rms1 is taken
    # on its FMA-formed object points, ~1e-7 relative away: see test_noise_free_problems_refine_to_the_planted_pose)
    ck = oref.cost(p3[use], p2[use], oref.cam_of(p["K"]), R1, t1)
    assert ck <= co * (1 + 1e-9), (ck, co)
    assert abs(rms1 ** 2 * use.sum() - ck) <= 1e-6 * ck


@gpu
def test_refined_poses_agree_with_the_oracle_on_the_kernels_consensus_set():
    rng = np.random.default_rng(40)
    six = None
    for _ in range(20):                         # 6 true correspondences + 2 outliers: RANSAC keeps exactly the 6
        cand = _problem(rng, 8, n_out=2, noise=0.5)
        r = _run(_dev([cand]))
        if r[3][0] and round(r[2][0] * 8) == 6:
            six = cand
            break
    assert six is not None
    probs = [_problem(rng, 3500, n_out=1050, noise=0.5), _problem(rng, 3500, n_out=1050, noise=0.5), _problem(rng, 64, n_out=16, noise=0.5),
             _problem(rng, 64, noise=0.5)]
    args = _dev(probs + [six])
    rot0, tvec0, ratio0, ok0, _ = _run(args)
    rot1, tvec1, ratio1, ok1, npts, st, mask = _run(args, refine="lm", return_inliers=True)
    assert ok1.all() and mask[-1].sum() == 6
    for i, p in enumerate(probs + [six]):
        _oracle_check(p, rot0[i], tvec0[i], mask[i], rot1[i], tvec1[i], st["rms_after"][i])


@gpu
def test_refinement_never_raises_the_reprojection_error():
    rng = np.random.default_rng(50)
    b = make_batch(rng, 200, 400, 0.3, 0.7)
    rot0, tvec0, ratio0, ok0, _ = _run(_batch_dev(b))
    rot1, tvec1, ratio1, ok1, npts, st, mask = _run(_batch_dev(b), refine="lm", return_inliers=True)
    assert ok1.all() and np.all(st["rms_after"] <= st["rms_before"])
    for i, p in enumerate(_unbatch(b)):
        p3, p2 = oref.problem_points(p)
        use = mask[i, :len(p3)]
        cam = oref.cam_of(p["K"])
        before, after = oref.rms(p3[use], p2[use], cam, rot0[i], tvec0[i]), oref.rms(p3[use], p2[use], cam, rot1[i], tvec1[i])
        assert after <= before * (1 + 1e-12), (i, before, after)         # (host sums: another order, the same fp64 terms)
        assert abs(before - st["rms_before"][i]) <= 1e-6 * before and abs(after - st["rms_after"][i]) <= 1e-6 * before   # (FMA-formed points)


@gpu
def test_refinement_improves_the_median_pose_error():
    rng = np.random.default_rng(60)
    b = make_batch(rng, 200, 3500, 0.3, 1.0)
    rot0, tvec0, _, ok0, _ = _run(_batch_dev(b))
    rot1, tvec1, _, ok1, _, st = _run(_batch_dev(b), refine="lm")
    assert ok0.all() and ok1.all()
    a0, t0 = pose_errors(rot0, tvec0, b["R"], b["t"])
    a1, t1 = pose_errors(rot1, tvec1, b["R"], b["t"])
    ra, rt = np.median(a1) / np.median(a0), np.median(t1) / np.median(t0)
    print(f"median rotation error {np.median(a0):.5f} -> {np.median(a1):.5f} deg (x{ra:.3f}); median relative translation error "
          f"{np.median(t0):.3e} -> {np.median(t1):.3e} (x{rt:.3f}); mean LM steps {st['iterations'].mean():.2f}")
    assert ra <= 1.0 and rt <= 1.0


@gpu
def test_standalone_refinement_on_a_ragged_batch():
    from pnp_problems import K0, random_rotations

    from picopose_amd.utils.pose_recovery import solve_pnp_refine_lm

    rng = np.random.default_rng(70)
    counts = [6, 64, 4096, 5, 64, 4096]
    noise = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    P, Nmax = len(counts), max(counts)
    R = random_rotations(rng, P)
    t = np.array([0.05, -0.03, 0.9]) + 0.05 * rng.standard_normal((P, 3))
    obj = (rng.random((P, Nmax, 3)) - 0.5) * 0.2
    pc = np.einsum("pnk,pjk->pnj", obj, R) + t[:, None]
    img = np.stack([K0[0, 2] + K0[0, 0] * pc[..., 0] / pc[..., 2], K0[1, 2] + K0[1, 1] * pc[..., 1] / pc[..., 2]], axis=-1)
    img += np.array(noise)[:, None, None] * rng.standard_normal(img.shape)
    for p, c in enumerate(counts):
        obj[p, c:], img[p, c:] = 1e30, np.nan          # rows beyond a problem's count are never read
    ax = rng.standard_normal((P, 3))
    w = np.radians(2.0) * ax / np.linalg.norm(ax, axis=1, keepdims=True)
    R0 = np.stack([oref.so3_exp(w[p]) @ R[p] for p in range(P)])
    dt = rng.standard_normal((P, 3))
    t0 = t + 0.01 * dt / np.linalg.norm(dt, axis=1, keepdims=True)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rot, tvec, st = solve_pnp_refine_lm(cuda(obj), cuda(img), cuda(K0), cuda(R0), cuda(t0), counts=cuda(np.array(counts, np.int32)))
    for p, c in enumerate(counts):
        if c < 6:      # under the minimum: the start, unchanged
            assert np.array_equal(rot[p], R0[p]) and np.array_equal(tvec[p, :, 0], t0[p]) and st["iterations"][p] == 0
            assert st["rms_before"][p] == st["rms_after"][p]
            continue
        assert st["iterations"][p] > 0 and st["rms_after"][p] <= st["rms_before"][p]
        if noise[p] == 0.0:
            assert np.abs(rot[p] - R[p]).max() < 1e-9 and np.abs(tvec[p, :, 0] - t[p]).max() < 1e-9 * np.linalg.norm(t[p])
            assert st["rms_after"][p] < 1e-6
        else:
            Ro, to, co, _ = oref.refine_lm(obj[p, :c], img[p, :c], oref.cam_of(K0), R0[p], t0[p])
            assert np.abs(rot[p] - Ro).max() < 1e-7 and np.abs(tvec[p, :, 0] - to).max() < 1e-7
            assert st["rms_after"][p] ** 2 * c <= co * (1 + 1e-9)         # (f64 inputs: the same data as the oracle's)


@gpu
def test_refining_launches_are_deterministic():
    rng = np.random.default_rng(80)
    args = _batch_dev(make_batch(rng, 32, 3500, 0.3, 0.5))
    a = _run(args, refine="lm", return_inliers=True)
    b = _run(args, refine="lm", return_inliers=True)
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert all(np.array_equal(x[k], y[k]) for k in x)
        else:
            assert np.array_equal(x, y)


@gpu
def test_pipeline_refines_without_reordering_hypotheses():
    import bench
    from picopose_amd.picopose import Net
    from picopose_amd.pipeline import (_rank_hypotheses, infer_batch, pnp_collect, pnp_for_outputs, pnp_for_outputs_async, pnp_inputs)
    from picopose_amd.utils.pose_recovery import pose_recovery_ransac_pnp_batched

    vit, hyp = "dinov2_vits14", 3
    net = Net(bench.make_cfg(vit))
    bench.seeded_weights(net, 4, vit)
    net = net.cuda().eval()
    ep = bench.make_end_points(1, 4, "cuda", 11)          # (the smoke test's model and inputs)
    with torch.no_grad():
        ep["template_feature"] = torch.stack([net.feature_extractor(ep["tem_rgb"][0])[-1]])
        plain = infer_batch(net, ep, hyp)
        refined = infer_batch(net, ep, hyp, pnp_refine="lm")
        outputs = net(ep, hyp)
    for a, b in zip(plain, refined):
        assert [h["inliers_ratio"] for h in a] == [h["inliers_ratio"] for h in b]
        assert [h["pnp_success"] for h in a] == [h["pnp_success"] for h in b]
    B = ep["real_K"].shape[0]
    rot, tvec, ratio, ok, st = pose_recovery_ransac_pnp_batched(*pnp_inputs(outputs, ep["real_K"]), refine="lm")
    assert ok.any() and np.all(st["rms_after"] <= st["rms_before"])
    stage2 = np.stack([o["pred_poses"].cpu().numpy() for o in outputs])
    expect = _rank_hypotheses(stage2, rot.reshape(hyp, B, 3, 3), tvec.reshape(hyp, B, 3, 1), ratio.reshape(hyp, B), ok.reshape(hyp, B), hyp)
    for a, b in zip(refined, expect):
        for x, y in zip(a, b):
            assert np.array_equal(x["R"], y["R"]) and np.array_equal(x["t"], y["t"]) and x["inliers_ratio"] == y["inliers_ratio"]
    sync = pnp_for_outputs(outputs, ep["real_K"], pnp_refine="lm")
    side = torch.cuda.Stream()
    asyn = pnp_collect(pnp_for_outputs_async(outputs, ep["real_K"], stream=side, pnp_refine="lm"), hyp, B)
    for x, y in zip(sync, asyn):
        assert np.array_equal(x, y)
    assert np.array_equal(sync[0], rot.reshape(hyp, B, 3, 3))
