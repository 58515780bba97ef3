"""Numpy float64 statement of the depth refinement contract of include/picopose_hip.h ("DEPTH REFINEMENT"), written from that text on
render_oracle.Triangles: the windowed render that keeps the face word (zbuffer), one linearisation (linearise), the pseudo-inverse step
through numpy.linalg.eigh (step), the loop with its stopping rules (run), and the test scenes.  It is checked against closed-form
answers in tests/test_depth_refine_cpu.py; the kernels are held to it in tests/test_depth_refine_gpu.py."""
import functools
import math

import numpy as np

import render_oracle as ro
import vsd_oracle as vo

F = np.float32
STRIP_ROWS = 8
DEFAULTS = dict(iterations=10, max_distance=100.0, min_points=1000, min_cos=0.1, rcond=1e-6, eps=1e-2, margin=32, max_translation=100.0,
                max_rotation=0.5, near=1.0)
U64 = 2.0 ** -53


def f32(v):
    """A parameter as the float32 number the kernel is given, in float64."""
    return float(F(v))


def zbuffer(vertices, faces, pose, K4, H, W, near=1.0, window=None):
    """vsd_oracle.depth32 keeping the face word -> ((H, W) float32 Z, 0 = background; (H, W) int64 face, -1 = background)."""
    x0, y0, x1, y1 = vo.full(H, W) if window is None else window
    z, face = np.zeros(H * W, dtype=F), np.full(H * W, -1, dtype=np.int64)
    if x1 <= x0 or y1 <= y0:
        return z.reshape(H, W), face.reshape(H, W)
    tri = ro.Triangles(vertices, faces, np.asarray(pose, dtype=F), tuple(F(k) for k in K4), H, W, near)
    tri.bx0, tri.bx1 = np.maximum(tri.bx0, x0), np.minimum(tri.bx1, x1 - 1)
    tri.by0, tri.by1 = np.maximum(tri.by0, y0), np.minimum(tri.by1, y1 - 1)
    tri.keep = tri.keep & (tri.bx0 <= tri.bx1) & (tri.by0 <= tri.by1)
    zbuf = np.full(H * W, ro.BG, dtype=np.uint64)
    for pix, fc, zz in tri.fragments(H, W):
        np.minimum.at(zbuf, pix, (zz.view(np.uint32).astype(np.uint64) << np.uint64(32)) | fc.astype(np.uint64))
    hit = zbuf != ro.BG
    z[hit] = (zbuf[hit] >> np.uint64(32)).astype(np.uint32).view(F)
    face[hit] = (zbuf[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return z.reshape(H, W), face.reshape(H, W)


def box_centre(vertices):
    v = np.asarray(vertices, dtype=F).astype(np.float64)
    return (v.min(axis=0) + v.max(axis=0)) / 2


def grow(window, margin, H, W):
    x0, y0, x1, y1 = window
    if x1 <= x0 or y1 <= y0:
        return (0, 0, 0, 0)
    return (max(x0 - margin, 0), max(y0 - margin, 0), min(x1 + margin, W), min(y1 + margin, H))


def linearise(pose32, obj, K4, depth_mm, window, max_distance=100.0, min_cos=0.1, near=1.0, return_abs=False):
    """Items 1 and 2 for one pose -> (sums (29,) float64 = 21 upper entries of J^T J, 6 of J^T r, sum r^2, N; N; fragile): fragile
    counts the associated samples whose min_cos or normal-flip decision lies within float64 rounding of its threshold (and those
    whose |m| is within rounding of 0).  obj: {"vertices", "faces", "info": {"diameter"}}; depth_mm (H, W) float32.
    return_abs: also the sums of the absolute values of the terms."""
    P = np.asarray(pose32, dtype=F)
    H, W = depth_mm.shape
    verts, faces = np.asarray(obj["vertices"], dtype=F), np.asarray(obj["faces"])
    z_r, face = zbuffer(verts, faces, P, K4, H, W, near, window)
    z_t = np.asarray(depth_mm, dtype=F)
    with np.errstate(invalid="ignore"):
        ok = (face >= 0) & (z_t > 0)
        ok &= np.abs(z_t - z_r) <= F(max_distance)                # the gate, float32
    y, x = np.nonzero(ok)
    fx, fy, cx, cy = (float(F(k)) for k in K4)
    R, t = P[:3, :3].astype(np.float64), P[:3, 3].astype(np.float64)
    v64 = verts.astype(np.float64)
    tri = faces[face[y, x]]
    cr = np.cross(v64[tri[:, 1]] - v64[tri[:, 0]], v64[tri[:, 2]] - v64[tri[:, 0]])
    m = cr @ R.T
    ln = np.linalg.norm(m, axis=1)
    good = np.any(cr != 0, axis=1) & (ln > 0)
    xr, yr = (x - cx) / fx, (y - cy) / fy
    zr, zt = z_r[y, x].astype(np.float64), z_t[y, x].astype(np.float64)
    pm, pt = np.stack([zr * xr, zr * yr, zr], axis=1), np.stack([zt * xr, zt * yr, zt], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = m / ln[:, None]
        dot = np.einsum("ij,ij->i", n, pm)
        flip = dot > 0
        n = np.where(flip[:, None], -n, n)
        dot = np.where(flip, -dot, dot)
        rng = np.linalg.norm(pm, axis=1)
        cosang = -dot / rng
        keep = good & ~(cosang < f32(min_cos))
    scale = np.maximum(rng, 1.0)
    fragile = int((good & ((np.abs(cosang - f32(min_cos)) <= 64 * U64) | (np.abs(dot) <= 64 * U64 * scale))).sum())
    n, pm, pt = n[keep], pm[keep], pt[keep]
    r = np.einsum("ij,ij->i", n, pt - pm)
    c = R @ box_centre(verts) + t
    rho = float(F(obj["info"]["diameter"])) / 2
    J = np.concatenate([np.cross(pm - c, n) / rho, n], axis=1)
    iu = np.triu_indices(6)
    terms = np.concatenate([J[:, iu[0]] * J[:, iu[1]], J * r[:, None], (r * r)[:, None], np.ones((len(r), 1))], axis=1)
    sums = np.array([math.fsum(col) for col in terms.T]) if len(r) else np.zeros(29)
    N = int(len(r))
    if return_abs:
        return sums, N, fragile, np.abs(terms).sum(axis=0) if N else np.zeros(29)
    return sums, N, fragile


def exp_so3(th):
    a2 = float(th @ th)
    a = math.sqrt(a2)
    A, B = (1 - a2 / 6, 0.5 - a2 / 24) if a2 < 1e-12 else (math.sin(a) / a, (1 - math.cos(a)) / a2)
    K = np.array([[0, -th[2], th[1]], [th[2], 0, -th[0]], [-th[1], th[0], 0]])
    return np.eye(3) + A * K + B * (K @ K)


def step(sums, pose32=None, obj=None, rcond=1e-6, full=False):
    """Item 3 -> (pose32 (4, 4) float32, rank).  full: also {"x" (6,): (rho theta, v), "cut_margin": the smallest |lambda / cut - 1|
    over the eigenvalues (inf when the cut is 0), "eig"}."""
    P = np.asarray(pose32, dtype=F)
    iu = np.triu_indices(6)
    A = np.zeros((6, 6))
    A[iu] = sums[:21]
    A = A + np.triu(A, 1).T
    lam, E = np.linalg.eigh(A)
    cut = f32(rcond) * lam.max()
    kept = (lam > 0) & (lam >= cut)
    g = np.asarray(sums[21:27], dtype=np.float64)
    x = sum((E[:, i] * (E[:, i] @ g) / lam[i] for i in np.nonzero(kept)[0]), np.zeros(6))
    R, t = P[:3, :3].astype(np.float64), P[:3, 3].astype(np.float64)
    c = R @ box_centre(obj["vertices"]) + t
    rho = float(F(obj["info"]["diameter"])) / 2
    Ex = exp_so3(x[:3] / rho)
    out = P.copy()
    out[:3, :3] = (Ex @ R).astype(F)
    out[:3, 3] = (c + Ex @ (t - c) + x[3:]).astype(F)
    rank = int(kept.sum())
    if full:
        with np.errstate(divide="ignore", invalid="ignore"):
            margin = float(np.min(np.abs(lam / cut - 1))) if cut > 0 else math.inf
        return out, rank, {"x": x, "cut_margin": margin, "eig": lam}
    return out, rank


def drift(pose32, pose_in32):
    """(|t - t_in|, angle(R R_in^T)) of two float32 poses, float64."""
    A, B = np.asarray(pose32, dtype=F).astype(np.float64), np.asarray(pose_in32, dtype=F).astype(np.float64)
    tr = float(np.sum(A[:3, :3] * B[:3, :3]))
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3])), math.acos(min(1.0, max(-1.0, 0.5 * (tr - 1.0))))


def run(pose32, obj, K4, depth_mm, window, iterations=10, max_distance=100.0, min_points=1000, min_cos=0.1, rcond=1e-6, eps=1e-2,
        max_translation=100.0, max_rotation=0.5, near=1.0, **_):
    """The loop with item 4 -> {"pose", "status", "iterations", "rank", "n_points", "rms_before", "rms_after", "trajectory", "fragile",
    "cut_margin" (per step)}.  `window`: the grown, clipped window of the INPUT pose."""
    P0 = np.asarray(pose32, dtype=F)
    out = {"pose": P0.copy(), "status": 4, "iterations": 0, "rank": 0, "n_points": 0, "rms_before": math.nan, "rms_after": math.nan,
           "trajectory": [P0.copy()], "fragile": [], "cut_margin": []}
    x0, y0, x1, y1 = window
    if not np.all(np.isfinite(P0[:3])) or x1 <= x0 or y1 <= y0:
        out["trajectory"] += [P0.copy()] * iterations
        return out
    P, status = P0.copy(), 1
    for it in range(iterations):
        sums, N, frag = linearise(P, obj, K4, depth_mm, window, max_distance, min_cos, near)
        rms = math.sqrt(sums[27] / N) if N else math.nan
        if it == 0:
            out["rms_before"] = rms
        out.update(rms_after=rms, n_points=N, iterations=it + 1)
        out["fragile"].append(frag)
        if N < min_points:
            status, P, out["rank"] = 2, P0.copy(), 0
            out["cut_margin"].append(math.inf)
        else:
            Pn, rank, info = step(sums, P, obj, rcond, full=True)
            out["rank"] = rank
            out["cut_margin"].append(info["cut_margin"])
            dt, ang = drift(Pn, P0)
            if not dt <= f32(max_translation) or not ang <= f32(max_rotation):
                status, P = 3, P0.copy()
            else:
                P = Pn
                if max(np.linalg.norm(info["x"][:3]), np.linalg.norm(info["x"][3:])) < f32(eps):
                    status = 0
        out["trajectory"].append(P.copy())
        if status != 1:
            break
    out["trajectory"] += [P.copy()] * (iterations + 1 - len(out["trajectory"]))
    out.update(pose=P, status=status)
    return out


def mssd(obj, pose_a, pose_b):
    """max over the vertices of |A x - B x| (no symmetries), float64."""
    v = np.asarray(obj["vertices"], dtype=np.float64)
    A, B = np.asarray(pose_a, dtype=np.float64), np.asarray(pose_b, dtype=np.float64)
    return float(np.linalg.norm((v @ A[:3, :3].T + A[:3, 3]) - (v @ B[:3, :3].T + B[:3, 3]), axis=1).max())


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def plan(obj, pose32, K4, H, W, margin=32, near=1.0):
    """evaluation.plan_window grown by the margin (the module under test plans the same window; test_depth_refine_cpu.py compares them)."""
    from picopose_amd.evaluation import plan_window

    v = np.asarray(obj["vertices"], dtype=F).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    return grow(plan_window(corners, np.asarray(pose32, dtype=F), tuple(float(F(k)) for k in K4), H, W, float(F(near))), margin, H, W)


@functools.lru_cache(maxsize=None)
def mixed():
    """vsd_oracle.mixed_scene (cube, icosphere and plate, two cameras, uint16 depth with occluders and a missing block): the scene,
    its depth in millimetres as the kernel sees it, and each estimate's window.  Shared, never modified."""
    scene = vo.mixed_scene()
    dm = vo.depth_mm32(scene["depth_u16"], scene["depth_scale"])
    poses = [vo.pose(R, t) for R, t in zip(scene["R_est"], scene["t_est"])]
    wins = [plan(scene["objects"][o], poses[p], vo.CAMS[scene["image_index"][p]], vo.H, vo.W) for p, o in enumerate(scene["obj_ids"].tolist())]
    return scene, dm, poses, wins


MIXED_PARAMS = dict(DEFAULTS, min_points=50)                      # the 90 x 120 scenes hold a few hundred samples per object


@functools.lru_cache(maxsize=None)
def mixed_runs():
    """oracle.run for every estimate of the mixed scene (MIXED_PARAMS)."""
    scene, dm, poses, wins = mixed()
    return [run(poses[p], scene["objects"][o], vo.CAMS[scene["image_index"][p]], dm[scene["image_index"][p]], wins[p], **MIXED_PARAMS)
            for p, o in enumerate(scene["obj_ids"].tolist())]


@functools.lru_cache(maxsize=None)
def convergence_scene(seed=5):
    """Per object (cube, icosphere) two ground truths in one 90 x 120 image each; test depth = the ground truths' oracle renders over a wall
    at 1500 mm (float millimetres); starts displaced 20 mm along the viewing ray, the cube also rotated by 3 degrees."""
    rng = np.random.default_rng(seed)
    objs = vo.objects()
    rows, depth = [], np.full((2, vo.H, vo.W), 1500.0, dtype=F)
    for o, im, tg in ((1, 0, (-60.0, -10.0, 480.0)), (2, 0, (70.0, 15.0, 520.0)), (1, 1, (40.0, 20.0, 560.0)), (2, 1, (-70.0, -15.0, 450.0))):
        Rg, tg = vo.random_rotation(rng), np.array(tg)
        Pg = vo.pose(Rg, tg)
        z, _ = zbuffer(objs[o]["vertices"], objs[o]["faces"], Pg, vo.CAMS[im], vo.H, vo.W)
        depth[im] = np.where(z > 0, z, depth[im])
        ray = tg / np.linalg.norm(tg)
        Re = vo.random_rotation(rng, math.radians(3.0)) @ Rg if o == 1 else Rg
        Ps = vo.pose(Re, tg + 20.0 * ray * (1 if len(rows) % 2 else -1))
        rows.append((o, im, Ps, Pg))
    return {"objects": objs, "obj_ids": np.array([r[0] for r in rows]), "image_index": np.array([r[1] for r in rows], dtype=np.int32),
            "start": np.stack([r[2] for r in rows]), "gt": np.stack([r[3] for r in rows]), "depth_mm": depth, "K": vo.k33(vo.CAMS)}


CONV_PARAMS = dict(DEFAULTS, min_points=50)


@functools.lru_cache(maxsize=None)
def convergence_runs():
    sc = convergence_scene()
    out = []
    for p, o in enumerate(sc["obj_ids"].tolist()):
        im = int(sc["image_index"][p])
        win = plan(sc["objects"][o], sc["start"][p], vo.CAMS[im], vo.H, vo.W)
        out.append(run(sc["start"][p], sc["objects"][o], vo.CAMS[im], sc["depth_mm"][im], win, **CONV_PARAMS))
    return out
