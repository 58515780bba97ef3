"""CPU oracle of the Levenberg-Marquardt pose refinement (pp_pnp_ransac_refine, pp_pnp_refine_lm) — test helper, numpy only.

The kernel's cost: sum over a point set of the squared pixel reprojection error, K's fu, fv, uc, vc, fp64.  This oracle minimises
the same cost from the same start to FULL convergence (Gauss-Newton steps with Levenberg-Marquardt damping until the step or the
cost decrease reaches rounding), with the rotation updated through the exponential map — the kernel uses the Cayley map, which
agrees to first order, so the two follow different paths to the same minimum.

Also builds problems in the batched PnP's input layout (tests/pnp_problems.py) whose float32 data is EXACTLY consistent with a
planted pose: the ground truth is then the minimum of the cost to fp64 rounding, which float32-rounded random problems do not allow
(their pixels carry ~1e-5 px of rounding, which moves the optimum ~1e-7 away from the planted pose)."""
import numpy as np

from pnp_problems import H, W


def cam_of(K):
    K = np.asarray(K, np.float64)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def residuals(p3, p2, cam, R, t):
    """-> r (n,2) px, camera-frame points (n,3)."""
    fu, fv, uc, vc = cam
    pc = np.asarray(p3, np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64).reshape(1, 3)
    r = np.stack([uc + fu * pc[:, 0] / pc[:, 2], vc + fv * pc[:, 1] / pc[:, 2]], axis=1) - np.asarray(p2, np.float64)
    return r, pc


def cost(p3, p2, cam, R, t):
    r, pc = residuals(p3, p2, cam, R, t)
    return float((r * r).sum()) if np.all(pc[:, 2] > 0) else float("inf")


def rms(p3, p2, cam, R, t):
    return float(np.sqrt(cost(p3, p2, cam, R, t) / max(len(p3), 1)))


def jacobian(p3, p2, cam, R, t):
    """-> r (2n,), J (2n,6): d r / d(w, v) for R <- exp([w]x) R, t <- t + v, at w = v = 0."""
    fu, fv, uc, vc = cam
    q = np.asarray(p3, np.float64) @ np.asarray(R, np.float64).T
    r, pc = residuals(p3, p2, cam, R, t)
    iz = 1.0 / pc[:, 2]
    n = len(q)
    dproj = np.zeros((n, 2, 3))
    dproj[:, 0, 0], dproj[:, 0, 2] = fu * iz, -fu * pc[:, 0] * iz * iz
    dproj[:, 1, 1], dproj[:, 1, 2] = fv * iz, -fv * pc[:, 1] * iz * iz
    dpw = np.zeros((n, 3, 3))                 # d(w x q)/dw = -[q]x
    dpw[:, 0, 1], dpw[:, 0, 2] = q[:, 2], -q[:, 1]
    dpw[:, 1, 0], dpw[:, 1, 2] = -q[:, 2], q[:, 0]
    dpw[:, 2, 0], dpw[:, 2, 1] = q[:, 1], -q[:, 0]
    J = np.concatenate([dproj @ dpw, dproj], axis=2)          # (n,2,6)
    return r.reshape(-1), J.reshape(-1, 6)


def so3_exp(w):
    th = float(np.linalg.norm(w))
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + Wx
    return np.eye(3) + np.sin(th) / th * Wx + (1.0 - np.cos(th)) / th ** 2 * (Wx @ Wx)


def refine_lm(p3, p2, cam, R, t, max_iters=500):
    """Minimise the cost from (R, t) to full convergence -> (R (3,3), t (3,), cost, accepted steps)."""
    R, t = np.array(R, np.float64), np.array(t, np.float64).reshape(3)
    c = cost(p3, p2, cam, R, t)
    lam, acc, rejected = 1e-3, 0, 0
    for _ in range(max_iters):
        r, J = jacobian(p3, p2, cam, R, t)
        A, g = J.T @ J, J.T @ r
        while True:
            dx = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
            Rn, tn = so3_exp(dx[:3]) @ R, t + dx[3:]
            cn = cost(p3, p2, cam, Rn, tn)
            if cn < c:
                break
            lam *= 10.0
            rejected += 1
            if np.linalg.norm(dx) < 1e-15 or rejected > 60:
                return R, t, c, acc
        dec, step = c - cn, np.linalg.norm(dx)
        R, t, c, acc, rejected = Rn, tn, cn, acc + 1, 0
        lam = max(lam / 10.0, 1e-15)
        if dec <= 1e-15 * c or step < 1e-15:
            break
    return R, t, c, acc


def signed_permutations(rng, P):
    """P random proper rotations with entries in {-1, 0, 1}: R X is exact in float32."""
    out = []
    while len(out) < P:
        M = np.eye(3)[rng.permutation(3)] * rng.choice([-1.0, 1.0], size=(3, 1))
        if np.linalg.det(M) > 0:
            out.append(M)
    return np.stack(out)


def exact_problem_arrays(rng, n, R, t):
    """n correspondences (object points (n,3), pixels (n,2)) that the pose (R, t) maps onto each other EXACTLY in float32, under
    K_EXACT: camera points on dyadic depths and rays whose pixels are multiples of 1/4 px, object points R^T (Pc - t)."""
    z = rng.choice([0.625, 0.75, 0.875, 1.0], size=n)
    k, l = rng.integers(-400, 401, size=n), rng.integers(-400, 401, size=n)
    pc = np.stack([k * z / 2048.0, l * z / 2048.0, z], axis=1)            # u = 320 + k / 4, v = 256 + l / 4
    obj = (pc - t[None]) @ R                                              # R^T (pc - t), exact for a signed permutation
    uv = np.stack([K_EXACT[0, 2] + k / 4.0, K_EXACT[1, 2] + l / 4.0], axis=1)
    assert np.array_equal(obj.astype(np.float32).astype(np.float64), obj) and np.array_equal(uv.astype(np.float32), uv)
    return obj, uv


K_EXACT = np.array([[512.0, 0.0, 320.0], [0.0, 512.0, 256.0], [0.0, 0.0, 1.0]])


def layout(rng, obj, uv, K=K_EXACT):
    """One problem in the batched PnP's input layout (tests/pnp_problems.make_batch, P = 1 unstacked) with an identity template pose,
    so that the kernel's object-frame points are `obj` bit for bit."""
    n = len(obj)
    cells, tcells = rng.permutation(H * W)[:n], rng.permutation(H * W)[:n]
    slots = np.sort(rng.permutation(H * W)[:n])
    src3d = np.zeros((3, H * W), np.float32)
    tar2d = np.zeros((2, H * W), np.float32)
    src3d[:, cells] = obj.T
    tar2d[:, tcells] = uv.T
    tar_pts = -np.ones((H * W, 2), np.int64)
    src_pts = -np.ones((H * W, 2), np.int64)
    src_pts[slots] = np.stack([cells % W, cells // W], axis=-1)
    tar_pts[slots] = np.stack([tcells % W, tcells // W], axis=-1)
    return dict(tar2d=tar2d.reshape(2, H, W), src3d=src3d.reshape(3, H, W), K=np.asarray(K, np.float32), pose=np.eye(4, dtype=np.float32),
                tar_pts=tar_pts, src_pts=src_pts)


def exact_problem(rng, n):
    """-> (problem dict in the batched layout, R_gt, t_gt)."""
    R = signed_permutations(rng, 1)[0]
    t = np.array([rng.integers(-16, 17) / 256.0, rng.integers(-16, 17) / 256.0, 0.0])
    obj, uv = exact_problem_arrays(rng, n, R, t)
    return layout(rng, obj, uv), R, t


def problem_points(p):
    """The kernel's object-frame points and pixels of one problem (oracle.pnp.gather_valid) as float64."""
    from oracle.pnp import gather_valid

    p3, p2 = gather_valid(p["tar2d"], p["src3d"], p["pose"], p["tar_pts"], p["src_pts"])
    return p3.astype(np.float64), p2.astype(np.float64)
