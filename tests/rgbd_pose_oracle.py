"""float64 numpy restatement of pp_rgbd_ransac (include/picopose_hip.h, "RGB-D POSE RECOVERY") and a generator of planted problems.

The restatement follows the contract clause by clause — the same gather, the same hash draws, the same degeneracy rule, the pairs
stored as float32 — but fits rigid motions by SVD with the determinant correction (Kabsch), deliberately another route than the
kernel's quaternion form: where the two agree, they agree on the least-squares fit and not on a shared derivation.

`margins` tells whether a problem's answer is fixed by the contract alone: no residual of any hypothesis or of the refit within
1e-7 inlier_dist of inlier_dist, no sample (and no refit) within a relative 1e-3 of a degeneracy bound.  With that margin rounding
cannot move a pair in or out of a consensus set, so kernel and oracle must report the same masks."""
import numpy as np

from oracle.pnp import hash32 as mix, sample_indices  # noqa: F401  (pp_pnp_ransac's rule: one mixer, one sampler)

MAXP, MAXH = 4096, 256
DEGENERATE = 1e-6
K0 = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1.0]], dtype=np.float32)
H = W = 64


def draw(prob, h, npts):
    """The 3 distinct indices of hypothesis h of problem `prob` (its index in the batch)."""
    return sample_indices(prob, h, npts, 3)


def gather(p, depth):
    """-> (ps (n,3) float32 object-frame source points, pq (n,3) float32 camera points, lidx (n,) listed index of each kept pair,
    num_listed).  p: one problem (tar2d, src3d, K, pose, tar_pts, src_pts, image); depth (n_images, dH, dW) float32."""
    tp, sp = p["tar_pts"], p["src_pts"]
    listed = np.flatnonzero((tp != -1).all(axis=1) & (sp != -1).all(axis=1))[:MAXP]
    n_images, dH, dW = depth.shape
    f32 = np.float32
    t2, s3, P = p["tar2d"].astype(f32), p["src3d"].astype(f32), p["pose"].astype(f32)
    tx, ty, sx, sy = tp[listed, 0], tp[listed, 1], sp[listed, 0], sp[listed, 1]
    u, v = t2[0, ty, tx], t2[1, ty, tx]
    with np.errstate(invalid="ignore"):
        xf, yf = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
        inside = (xf >= 0) & (xf < dW) & (yf >= 0) & (yf < dH)
    img = int(p["image"])
    if not 0 <= img < n_images:
        inside[:] = False
    xi, yi = np.where(inside, xf, 0).astype(np.int64), np.where(inside, yf, 0).astype(np.int64)
    z = np.where(inside, depth[img if 0 <= img < n_images else 0, yi, xi], f32(0)).astype(f32)
    keep = inside & np.isfinite(z) & (z > 0)
    # (X - t_tem) @ R_tem, float32 operations in that order
    d = (s3[:, sy, sx].T - P[:3, 3][None]).astype(f32)
    ps = ((d[:, 0:1] * P[0:1, :3]).astype(f32) + (d[:, 1:2] * P[1:2, :3]).astype(f32)).astype(f32)
    ps = (ps + (d[:, 2:3] * P[2:3, :3]).astype(f32)).astype(f32)
    K = p["K"].astype(f32).astype(np.float64)
    u64, v64, z64 = u.astype(np.float64), v.astype(np.float64), z.astype(np.float64)
    with np.errstate(invalid="ignore"):
        q = np.stack([(u64 - K[0, 2]) * z64 / K[0, 0], (v64 - K[1, 2]) * z64 / K[1, 1], z64], axis=1)
    return ps[keep], q[keep].astype(f32), np.flatnonzero(keep), len(listed)


def tri_measure(tri):
    """(|a x b|^2, 1e-6 |a|^2 |b|^2) of a (3,3) triangle's two edges from its first point."""
    a, b = tri[1] - tri[0], tri[2] - tri[0]
    c = np.cross(a, b)
    return float(c @ c), DEGENERATE * float(a @ a) * float(b @ b)


def rigid_fit(p, q):
    """Least-squares R, t with q ~ R p + t (Kabsch: SVD of the centred cross-covariance, determinant correction)."""
    pm, qm = p.mean(axis=0), q.mean(axis=0)
    Hm = (p - pm).T @ (q - qm)
    U, _, Vt = np.linalg.svd(Hm)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    return R, qm - R @ pm


def residuals2(R, t, ps, pq):
    d = ps @ R.T + t - pq
    return (d * d).sum(axis=1)


FAIL = dict(rot=np.eye(3), tvec=np.array([0.0, 0.0, 1.0]), ratio=0.0, ok=False, rms=0.0)


def solve(p, depth, prob, iterations=150, inlier_dist=None):
    """pp_rgbd_ransac for one problem at batch index `prob` -> dict(rot, tvec, ratio, ok, npts, nlisted, rms, mask (N,) bool) plus
    margin_dist / margin_deg: the smallest relative distance of any inlier / degeneracy decision from its bound (inf when none was
    taken), see `margins`."""
    N = p["tar_pts"].shape[0]
    ps32, pq32, lidx, nlisted = gather(p, depth)
    npts = len(ps32)
    out = dict(FAIL, npts=npts, nlisted=nlisted, mask=np.zeros(N, bool), margin_dist=np.inf, margin_deg=np.inf)
    dist = np.float32(p["inlier_dist"] if inlier_dist is None else inlier_dist)
    if npts < 3 or not dist > 0:
        return out
    ps, pq = ps32.astype(np.float64), pq32.astype(np.float64)
    dist = float(dist)
    th2 = dist * dist
    best_c, best = -1, None
    m_dist, m_deg = np.inf, np.inf
    for h in range(min(iterations, MAXH)):
        idx = draw(prob, h, npts)
        deg = False
        for tri in (ps[idx], pq[idx]):
            lhs, rhs = tri_measure(tri)
            deg |= lhs <= rhs
            m_deg = min(m_deg, abs(lhs - rhs) / rhs if rhs > 0 else (np.inf if lhs > 0 else 0.0))
        c, R, t = 0, None, None
        if not deg:
            R, t = rigid_fit(ps[idx], pq[idx])
            r2 = residuals2(R, t, ps, pq)
            with np.errstate(invalid="ignore"):
                c = int((r2 <= th2).sum())
            m_dist = min(m_dist, float(np.abs(np.sqrt(r2) - dist).min()) / dist)
        if c > best_c:
            best_c, best = c, (R, t)
    out.update(margin_dist=m_dist, margin_deg=m_deg)
    if best_c < 3:
        return out
    R, t = best
    use = residuals2(R, t, ps, pq) <= th2
    Rf, tf = rigid_fit(ps[use], pq[use])
    c = ps[use] - ps[use].mean(axis=0)
    lam = np.sort(np.linalg.eigvalsh(c.T @ c))[::-1]
    out["margin_deg"] = min(m_deg, abs(lam[1] - DEGENERATE * lam[0]) / (DEGENERATE * lam[0]))
    out["margin_dist"] = min(m_dist, float(np.abs(np.sqrt(residuals2(Rf, tf, ps, pq)) - dist).min()) / dist)
    if np.isfinite(Rf).all() and np.isfinite(tf).all() and not lam[1] <= DEGENERATE * lam[0]:
        R, t = Rf, tf
    mask = np.zeros(N, bool)
    mask[lidx[use]] = True
    out.update(rot=R, tvec=t, ratio=best_c / npts, ok=True, rms=float(np.sqrt(residuals2(R, t, ps[use], pq[use]).mean())), mask=mask)
    return out


def margins(result):
    """The margin check of a solved problem: every residual at least 1e-7 inlier_dist away from inlier_dist, every degeneracy
    decision a relative 1e-3 away from its bound (an exactly collinear sample, measure 0, is a relative 1 below it)."""
    return result["margin_dist"] > 1e-7 and result["margin_deg"] > 1e-3


# ------------------------------------------------------------------ planted problems
def random_rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def pack(rng, u, v, src, N=MAXP):
    """n pairs of a pixel (u, v) and a source point -> the layout the solvers consume: tar2d (2,H,W) and src3d (3,H,W) float32 maps
    with the pairs in random distinct cells, tar_pts / src_pts (N,2) int64 [x, y] lists in n random slots (ascending), -1 elsewhere."""
    n = len(u)
    f32 = np.float32
    cells, tcells = rng.permutation(H * W)[:n], rng.permutation(H * W)[:n]
    slots = np.sort(rng.permutation(N)[:n])
    src3d, tar2d = np.zeros((3, H * W), f32), np.zeros((2, H * W), f32)
    src3d[:, cells] = np.asarray(src).T.astype(f32)
    tar2d[0, tcells], tar2d[1, tcells] = u, v
    tar_pts, src_pts = -np.ones((N, 2), np.int64), -np.ones((N, 2), np.int64)
    src_pts[slots] = np.stack([cells % W, cells // W], axis=-1)
    tar_pts[slots] = np.stack([tcells % W, tcells // W], axis=-1)
    return dict(tar2d=tar2d.reshape(2, H, W), src3d=src3d.reshape(3, H, W), tar_pts=tar_pts, src_pts=src_pts)


class Scene:
    """n_images depth images (dH, dW) float32, 0 (missing) where no problem wrote; hands out pixels no other problem uses."""

    def __init__(self, rng, n_images=2, dH=120, dW=160):
        self.rng, self.depth = rng, np.zeros((n_images, dH, dW), np.float32)
        self.free = [list(rng.permutation(dH * dW)) for _ in range(n_images)]

    def take(self, image, n):
        got, self.free[image] = self.free[image][:n], self.free[image][n:]
        assert len(got) == n, "depth image full"
        return np.array(got, dtype=np.int64)


def make_problem(scene, n_listed, outlier_frac=0.0, noise=0.0, n_missing=0, n_outside=0, image=0, inlier_dist=0.005, collinear=False,
                 N=MAXP):
    """One problem with `n_listed` list entries (the rest of the N slots are -1): n_missing of them at pixels with depth 0, n_outside
    at pixels outside the image, of the others round(outlier_frac * n) with a random source point, and the remaining pairs
    consistent with a planted pose (R, t): the pixel's (u, v) carry sub-pixel offsets as float32, z is float32 and is written
    into scene.depth[image], tem_pose = I and the source point R^T (q - t) (+ Gaussian noise of std `noise`) is rounded to float32.
    collinear: every source point on one line (exactly, in float32)."""
    rng = scene.rng
    _, dH, dW = scene.depth.shape
    n_good = n_listed - n_missing - n_outside
    assert n_good >= 0 and n_listed <= N <= H * W
    f32 = np.float32
    pix = scene.take(image, n_good + n_missing)
    xi, yi = pix % dW, pix // dW
    u = (xi + rng.uniform(-0.45, 0.45, len(pix))).astype(f32)
    v = (yi + rng.uniform(-0.45, 0.45, len(pix))).astype(f32)
    z = rng.uniform(0.8, 1.0, len(pix)).astype(f32)
    z[n_good:] = 0                                               # missing depth (the pixel stays reserved)
    scene.depth[image, yi, xi] = z
    uo = np.where(rng.random(n_outside) < 0.5, rng.uniform(-40.0, -0.51, n_outside), rng.uniform(dW - 0.5, dW + 40.0, n_outside))
    u = np.concatenate([u, uo.astype(f32)])
    v = np.concatenate([v, rng.uniform(0, dH - 1, n_outside).astype(f32)])
    assert np.all((u[len(pix):] < f32(-0.5)) | (u[len(pix):] >= f32(dW - 0.5)))
    K = K0.astype(np.float64)
    zg = z[:n_good].astype(np.float64)
    q = np.stack([(u[:n_good].astype(np.float64) - K[0, 2]) * zg / K[0, 0], (v[:n_good].astype(np.float64) - K[1, 2]) * zg / K[1, 1], zg], axis=1)
    R = random_rotation(rng)
    t = (q.mean(axis=0) if n_good else np.array([0.0, 0.0, 0.9])) + 0.01 * rng.standard_normal(3)
    src = np.zeros((n_listed, 3))
    src[:n_good] = (q - t) @ R + noise * rng.standard_normal((n_good, 3))
    n_out = int(round(outlier_frac * n_good))
    src[:n_out] = (rng.random((n_out, 3)) - 0.5) * 0.3
    src[n_good:] = (rng.random((n_listed - n_good, 3)) - 0.5) * 0.3
    if collinear:
        src = rng.permutation(4096)[:n_listed, None] * np.array([1.0, 2.0, -1.0]) / 1024.0 - np.array([2.0, 4.0, -2.0])
    order = rng.permutation(n_listed)                           # outliers, missing and outside entries anywhere in the list
    u, v, src = u[order], v[order], src[order]
    maps = pack(rng, u, v, src, N)
    return dict(maps, K=K0.copy(), pose=np.eye(4, dtype=f32), image=image, inlier_dist=f32(inlier_dist), R=R, t=t, n_in=n_good - n_out)
