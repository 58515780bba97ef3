"""CPU: argument validation of the Levenberg-Marquardt pose refinement (Python API and the two C-ABI entries, before any device
work) and the self-check of its numpy oracle (tests/pnp_refine_oracle.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pnp_refine_oracle as oref  # noqa: E402

PP_EINVAL = -1


class _NoDevice:
    """Stands for an input tensor: any use of it (a device conversion, .shape, .contiguous) fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"device work ({name}) before the argument check")


@pytest.mark.parametrize("kw", [dict(refine="LM"), dict(refine="gn"), dict(refine=True), dict(refine_iters=0), dict(refine_iters=-3),
                                dict(refine_iters=2.5), dict(refine_iters=True), dict(refine_eps=-1e-9), dict(refine_eps=float("nan")),
                                dict(refine_eps=float("inf")), dict(refine_eps="1e-7"), dict(return_inliers=True)])
def test_bad_refine_arguments_raise_before_device_work(kw):
    from picopose_amd.utils import pose_recovery as pr

    x = _NoDevice()
    with pytest.raises(ValueError):
        pr.pnp_launch(x, x, x, x, x, x, **kw)
    with pytest.raises(ValueError):
        pr.pose_recovery_ransac_pnp_batched(x, x, x, x, x, x, **kw)
    with pytest.raises(ValueError):
        pr.pose_recovery_ransac_pnp_batched_async(x, x, x, x, x, x, **kw)
    with pytest.raises(ValueError):
        pr.pose_recovery_ransac_pnp(x, x, x, x, x, x, **kw)


def test_good_refine_arguments_pass_and_the_drop_in_keeps_six_positionals():
    import inspect

    from picopose_amd.utils import pose_recovery as pr

    assert pr.check_refine(None) is False and pr.check_refine("lm", 1, 0.0, True) is True
    assert pr.check_refine("lm", np.int64(5), np.float32(1e-6)) is True
    assert pr.REFINE_EPS == np.finfo(np.float32).eps
    sig = inspect.signature(pr.pose_recovery_ransac_pnp)
    pos = [p for p in sig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in pos] == ["tar_pts_2d", "src_pts_3d", "K", "tem_pose", "tar_pts", "src_pts"]
    assert all(sig.parameters[k].kind == inspect.Parameter.KEYWORD_ONLY for k in ("refine", "refine_iters", "refine_eps", "return_inliers"))


def test_solve_pnp_refine_lm_validates_before_device_work():
    import torch

    from picopose_amd.utils.pose_recovery import solve_pnp_refine_lm

    P, N = 2, 10
    o, i, K, R, t = torch.zeros(P, N, 3), torch.zeros(P, N, 2), torch.eye(3), torch.eye(3).repeat(P, 1, 1), torch.zeros(P, 3)
    for kw in (dict(max_iters=0), dict(max_iters=-1), dict(eps=-1.0), dict(eps=float("nan")), dict(counts=[1, 2, 3]),
               dict(counts=[-1, 4]), dict(counts=[4, N + 1])):
        with pytest.raises(ValueError):
            solve_pnp_refine_lm(o, i, K, R, t, **kw)
    for args in ((torch.zeros(P, N, 2), i, K, R, t), (o, torch.zeros(P, N + 1, 2), K, R, t), (o, i, torch.eye(4), R, t),
                 (o, i, K, torch.eye(3), t), (o, i, K, R, torch.zeros(P, 4)), (torch.zeros(P, 4097, 3), torch.zeros(P, 4097, 2), K, R, t),
                 (torch.zeros(P, 0, 3), torch.zeros(P, 0, 2), K, R, t)):
        with pytest.raises(ValueError):
            solve_pnp_refine_lm(*args)


def test_pipeline_rejects_bad_pnp_refine_before_device_work():
    from picopose_amd import pipeline

    with pytest.raises(ValueError):
        pipeline.infer_batch(_NoDevice(), _NoDevice(), pnp_refine="levenberg")
    with pytest.raises(ValueError):
        pipeline.infer_batch(_NoDevice(), _NoDevice(), pnp_fn=lambda o, k: None, pnp_refine="lm")
    with pytest.raises(ValueError):
        pipeline.infer_image(_NoDevice(), _NoDevice(), _NoDevice(), pnp_refine="LM")


def _buf():
    b = (ctypes.c_char * 64)()
    return ctypes.addressof(b) + (-ctypes.addressof(b)) % 16, b


def test_abi_entries_reject_bad_arguments_without_a_gpu():
    from picopose_amd import _lib

    L = _lib.lib()
    p, _keep = _buf()
    # pp_pnp_ransac_refine(6 inputs, P, H, W, N, iterations, threshold, max_iters, eps, rot, tvec, ratio, ok, npts, rms0, rms1, its, mask, stream)
    good = [p] * 6 + [2, 64, 64, 4096, 150, 2.0, 20, 1e-7] + [p] * 8 + [None, None]
    assert len(good) == len(L.pp_pnp_ransac_refine.argtypes)
    bad = []
    for k in list(range(6)) + list(range(14, 22)):           # every required pointer (the mask is optional)
        a = list(good)
        a[k] = None
        bad.append(a)
    for k, v in ((6, 0), (6, -1), (9, 0), (9, 4097), (12, 0), (12, -5), (13, -1e-12), (13, float("nan")), (10, 0), (11, 0.0)):
        a = list(good)
        a[k] = v
        bad.append(a)
    for a in bad:
        assert L.pp_pnp_ransac_refine(*a) == PP_EINVAL, a
    # pp_pnp_refine_lm(obj, img, count, K, rot0, tvec0, P, Nmax, max_iters, eps, rot, tvec, rms0, rms1, its, stream)
    good = [p] * 6 + [2, 64, 20, 1e-7] + [p] * 5 + [None]
    assert len(good) == len(L.pp_pnp_refine_lm.argtypes)
    bad = []
    for k in list(range(6)) + list(range(10, 15)):
        a = list(good)
        a[k] = None
        bad.append(a)
    for k, v in ((6, 0), (6, -2), (7, 0), (7, 4097), (8, 0), (8, -1), (9, -1.0), (9, float("nan"))):
        a = list(good)
        a[k] = v
        bad.append(a)
    for a in bad:
        assert L.pp_pnp_refine_lm(*a) == PP_EINVAL, a
    assert {"pp_pnp_ransac_refine", "pp_pnp_refine_lm"} <= set(_lib.declared_symbols())


def test_oracle_jacobian_matches_finite_differences():
    rng = np.random.default_rng(3)
    p3 = (rng.random((20, 3)) - 0.5) * 0.2
    R, t = oref.so3_exp(rng.standard_normal(3) * 0.5), np.array([0.02, -0.01, 0.9])
    cam = oref.cam_of(oref.K_EXACT)
    p2 = oref.residuals(p3, np.zeros((20, 2)), cam, R, t)[0] + rng.standard_normal((20, 2))
    r0, J = oref.jacobian(p3, p2, cam, R, t)
    h = 1e-7
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        rp = oref.residuals(p3, p2, cam, oref.so3_exp(d[:3]) @ R, t + d[3:])[0].reshape(-1)
        rm = oref.residuals(p3, p2, cam, oref.so3_exp(-d[:3]) @ R, t - d[3:])[0].reshape(-1)
        assert np.abs((rp - rm) / (2 * h) - J[:, k]).max() < 1e-4 * np.abs(J[:, k]).max()


@pytest.mark.parametrize("n", [6, 8, 64, 3500])
def test_oracle_converges_to_the_planted_pose_on_noise_free_problems(n):
    from pnp_problems import K0, make_batch

    rng = np.random.default_rng(100 + n)
    # random poses, fp64 data: the planted pose is the minimum (cost 0)
    b = make_batch(rng, 1, n)
    p3 = (rng.random((n, 3)) - 0.5) * 0.2
    R, t = b["R"][0], b["t"][0]
    cam = oref.cam_of(K0)
    p2 = oref.residuals(p3, np.zeros((n, 2)), cam, R, t)[0]
    R0, t0 = oref.so3_exp(np.radians(2.0) * rng.standard_normal(3) / np.sqrt(3)) @ R, t + 0.01 * rng.standard_normal(3) / np.sqrt(3)
    Rr, tr, c, acc = oref.refine_lm(p3, p2, cam, R0, t0)
    assert acc > 0 and np.abs(Rr - R).max() < 1e-10 and np.abs(tr - t).max() < 1e-10 * np.linalg.norm(t), (np.abs(Rr - R).max(), c)
    # the float32-exact construction of the GPU tests: also a zero-cost minimum at the planted pose
    p, Rg, tg = oref.exact_problem(rng, n)
    q3, q2 = oref.problem_points(p)
    assert len(q3) == n and oref.cost(q3, q2, oref.cam_of(p["K"]), Rg, tg) < 1e-20
    Rr, tr, c, _ = oref.refine_lm(q3, q2, oref.cam_of(p["K"]), oref.so3_exp(np.array([0.02, -0.01, 0.015])) @ Rg, tg + 0.005)
    assert np.abs(Rr - Rg).max() < 1e-10 and np.abs(tr - tg).max() < 1e-10 * max(np.linalg.norm(tg), 1.0)
