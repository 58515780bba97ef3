"""Numpy statement of the VSD contract of include/picopose_hip.h ("VSD, the Visible Surface Discrepancy"), written from that text and
built on render_oracle.Triangles: the windowed depth render (depth32), the float32 restatement of the pair reduction (vsd32), the
definition in float64 (vsd64), the pixels whose float64 margin is too small for float32 to decide (fragile), and the test scenes.
It is checked against closed-form answers in tests/test_vsd_cpu.py; the kernels are held to it in tests/test_vsd_gpu.py."""
import math

import numpy as np

import render_oracle as ro

F = np.float32
U32 = 2.0 ** -24
TAUS = np.arange(1, 11) / 20.0


def full(H, W):
    return (0, 0, W, H)


def depth32(vertices, faces, pose, K4, H, W, near=1.0, window=None):
    """Items 1-5, 7 and the Z of item 6 of the raster contract, sampled for x0 <= x < x1, y0 <= y < y1 of `window` (default: the
    frame) -> ((H, W) float32 camera Z, 0 = background; triangles dropped at the near plane).  An empty window renders and counts nothing."""
    x0, y0, x1, y1 = full(H, W) if window is None else window
    out = np.zeros(H * W, dtype=F)
    if x1 <= x0 or y1 <= y0:
        return out.reshape(H, W), 0
    tri = ro.Triangles(vertices, faces, np.asarray(pose, dtype=F), tuple(F(k) for k in K4), H, W, near)
    tri.bx0, tri.bx1 = np.maximum(tri.bx0, x0), np.minimum(tri.bx1, x1 - 1)
    tri.by0, tri.by1 = np.maximum(tri.by0, y0), np.minimum(tri.by1, y1 - 1)
    tri.keep = tri.keep & (tri.bx0 <= tri.bx1) & (tri.by0 <= tri.by1)
    zbuf = np.full(H * W, ro.BG, dtype=np.uint64)
    for pix, face, z in tri.fragments(H, W):
        np.minimum.at(zbuf, pix, (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | face.astype(np.uint64))
    hit = zbuf != ro.BG
    out[hit] = (zbuf[hit] >> np.uint64(32)).astype(np.uint32).view(F)
    return out.reshape(H, W), tri.near_count


def _rays32(K4, H, W):
    fx, fy, cx, cy = (F(k) for k in K4)
    xr = (np.arange(W, dtype=F)[None, :] - cx) / fx
    yr = (np.arange(H, dtype=F)[:, None] - cy) / fy
    return np.sqrt((xr * xr + yr * yr) + F(1))


def vsd32(z_est, z_gt, z_test, K4, diameter, delta=15.0, taus=TAUS):
    """The pair reduction in float32, operation by operation -> (counts (2 + T,) int64 = {union, inter, n_1 .. n_T}, e (T,) float32)."""
    z_est, z_gt, z_test = (np.asarray(a, dtype=F) for a in (z_est, z_gt, z_test))
    r = _rays32(K4, *z_est.shape)
    with np.errstate(invalid="ignore"):
        missing = ~(z_test > 0)
        d_est, d_gt, d_test = z_est * r, z_gt * r, z_test * r
        vis_gt = (d_gt > 0) & (missing | (d_gt - d_test <= F(delta)))
        vis_est = (d_est > 0) & (missing | (d_est - d_test <= F(delta)) | vis_gt)
        inter, union = vis_gt & vis_est, vis_gt | vis_est
        dd = np.abs(d_gt - d_est) / F(diameter)
        n = [int((inter & (dd >= F(t))).sum()) for t in np.asarray(taus, dtype=F)]
    u, i = int(union.sum()), int(inter.sum())
    e = [F((k + u - i) / u) if u else F(1) for k in n]          # (python floats: the float64 quotient, rounded once)
    return np.array([u, i] + n, dtype=np.int64), np.array(e, dtype=F)


def _terms64(z_est, z_gt, z_test, K4, diameter, delta):
    fx, fy, cx, cy = (float(F(k)) for k in K4)
    H, W = z_est.shape
    xr, yr = (np.arange(W, dtype=np.float64)[None, :] - cx) / fx, (np.arange(H, dtype=np.float64)[:, None] - cy) / fy
    r = np.sqrt(xr * xr + yr * yr + 1.0)
    z_test = np.asarray(z_test, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        missing = ~(z_test > 0)
    d_est, d_gt, d_test = z_est.astype(np.float64) * r, z_gt.astype(np.float64) * r, np.where(missing, 0.0, z_test) * r
    return missing, d_est, d_gt, d_test


def vsd64(z_est, z_gt, z_test, K4, diameter, delta=15.0, taus=TAUS):
    """Section 1 of the definition in float64 from given depth images (the float32 values the caller holds; the taus, delta and
    diameter as the float32 numbers the kernel is given) -> (counts, e float64)."""
    missing, d_est, d_gt, d_test = _terms64(np.asarray(z_est), np.asarray(z_gt), z_test, K4, diameter, delta)
    dl, dm = float(F(delta)), float(F(diameter))
    vis_gt = (d_gt > 0) & (missing | (d_gt - d_test <= dl))
    vis_est = (d_est > 0) & (missing | (d_est - d_test <= dl) | vis_gt)
    inter, union = vis_gt & vis_est, vis_gt | vis_est
    dd = np.abs(d_gt - d_est) / dm
    n = [int((inter & (dd >= float(F(t)))).sum()) for t in taus]
    u, i = int(union.sum()), int(inter.sum())
    return np.array([u, i] + n, dtype=np.int64), np.array([(k + u - i) / u if u else 1.0 for k in n])


def fragile(z_est, z_gt, z_test, K4, diameter, delta=15.0, taus=TAUS):
    """Per compared quantity the pixels float32 may decide differently from float64: those whose float64 margin is within
    8 * 2^-24 * max(D) millimetres (divided by the diameter for dd) -> (2 + T,) int64 counts for {union, inter, n_1 .. n_T}.  A pixel
    with a fragile visibility compare is fragile for every quantity; a pixel with a fragile dd compare for that tau only."""
    missing, d_est, d_gt, d_test = _terms64(np.asarray(z_est), np.asarray(z_gt), z_test, K4, diameter, delta)
    dl, dm = float(F(delta)), float(F(diameter))
    tol = 8 * U32 * np.maximum(np.maximum(d_est, d_gt), d_test)
    vis = ((d_gt > 0) & ~missing & (np.abs(d_gt - d_test - dl) <= tol)) | ((d_est > 0) & ~missing & (np.abs(d_est - d_test - dl) <= tol))
    both = (d_gt > 0) & (d_est > 0)
    dd = np.abs(d_gt - d_est) / dm
    n = [int((vis | (both & (np.abs(dd - float(F(t))) <= tol / dm))).sum()) for t in taus]
    return np.array([int(vis.sum())] * 2 + n, dtype=np.int64)


# ---- meshes and scenes ---------------------------------------------------------------------------------------------------------------
def plate(n, px_mm=5.0):
    """A square of side n * px_mm millimetres in the plane z = 0: at Z = 500 under f = 100 it covers n x n samples."""
    h = F(n * px_mm / 2)
    return {"vertices": np.array([[-h, -h, 0], [h, -h, 0], [-h, h, 0], [h, h, 0]], dtype=F), "faces": np.array([[0, 1, 3], [0, 3, 2]], dtype=np.int32)}


PLATE_N = 16
PLATE_K4 = (100.0, 100.0, 40.5, 30.5)                            # half-integer principal point: the plate's edges fall between samples
PLATE_HW = (61, 83)
PLATE_Z = 500.0
PLATE_DIAMETER = PLATE_N * 5.0 * math.sqrt(2.0)


def pose(R=np.eye(3), t=(0, 0, PLATE_Z)):
    P = np.eye(4, dtype=F)
    P[:3, :3], P[:3, 3] = R, t
    return P


def plate_cases():
    """The closed-form scenes: name -> (est pose, gt pose, test depth (H, W) float32 mm, expected {union, inter, e (T,)}) for the
    n = 16 plate, delta = 15, the default taus.  Derivations in tests/test_vsd_cpu.py."""
    n, (H, W) = PLATE_N, PLATE_HW
    x0, y0 = int(PLATE_K4[2] - n / 2 + 0.5), int(PLATE_K4[3] - n / 2 + 0.5)       # first covered column / row
    none = np.zeros((H, W), dtype=F)
    cases = {"identical": (pose(), pose(), none, {"union": n * n, "inter": n * n, "e": np.zeros(10)})}
    k = 3
    cases["shift"] = (pose(t=(5.0 * k, 0, PLATE_Z)), pose(), none, {"union": n * (n + k), "inter": n * (n - k), "e": np.full(10, 2 * k / (n + k))})
    occ = none.copy()
    occ[:, x0:x0 + n // 2] = 300.0                                # 200 mm in front of the left half
    cases["occluder"] = (pose(), pose(), occ, {"union": n * n // 2, "inter": n * n // 2, "e": np.zeros(10)})
    cases["behind"] = (pose(), pose(), np.full((H, W), 900.0, dtype=F), {"union": n * n, "inter": n * n, "e": np.zeros(10)})
    # estimate 30 mm behind a visible ground truth: D_est - D_test = 30 r > delta, visible through the visib_gt clause; dd = 30 r / d
    # with 1 <= r < 1.02: 0.2652 .. 0.2705, between the taus 0.25 and 0.30 with more than 1 % margin
    d = 30.0 / PLATE_DIAMETER
    cases["gt_clause"] = (pose(t=(0, 0, PLATE_Z + 30.0)), pose(), np.full((H, W), PLATE_Z, dtype=F),
                          {"union": n * n, "inter": n * n, "e": (TAUS <= d).astype(np.float64)})
    cases["offset"] = (pose(t=(0, 0, PLATE_Z + 30.0)), pose(), none, {"union": n * n, "inter": n * n, "e": (TAUS <= d).astype(np.float64)})
    cases["empty"] = (pose(t=(5000.0, 0, PLATE_Z)), pose(t=(-5000.0, 0, PLATE_Z)), none, {"union": 0, "inter": 0, "e": np.ones(10)})
    return cases


def random_rotation(rng, angle=None):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.uniform(0, math.pi) if angle is None else angle
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * k + (1 - math.cos(th)) * (k @ k)


H, W = 90, 120                                                    # no multiple of the 16 x 16 tile
CAMS = np.array([[100.0, 100.0, 59.5, 44.5], [130.0, 128.0, 63.25, 41.75]], dtype=F)


def objects():
    """obj_id -> {"vertices" (mm), "faces", "info"}: a cube (12 large triangles: the tiled path), an icosphere (1280 small ones: the
    per-lane path) and the plate."""
    c, s, p = ro.cube(40.0), ro.icosphere(3, 50.0), plate(PLATE_N)
    return {1: {"vertices": c["vertices"], "faces": c["faces"], "info": {"diameter": 80.0 * math.sqrt(3.0)}},
            2: {"vertices": s["vertices"], "faces": s["faces"], "info": {"diameter": 100.0}},
            3: {"vertices": p["vertices"], "faces": p["faces"], "info": {"diameter": PLATE_DIAMETER}}}


def mixed_scene(seed=3, per_object=4):
    """Two images (different K), per image and object `per_object` // 2 ground truths, each with one estimate a few millimetres and degrees
    away.  Test depth: the ground truths composited over a wall at 1500 mm, an occluder 60 mm in front of the left half of every other
    instance, a block of missing samples; stored as uint16 with depth_scale 0.5 -> dict of arrays."""
    rng = np.random.default_rng(seed)
    objs = objects()
    rows, depth = [], np.full((2, H, W), 1500.0, dtype=F)
    for o in (1, 2, 3):
        for j in range(per_object):
            im = j % 2
            Rg = random_rotation(rng) if o != 3 else random_rotation(rng, rng.uniform(0, 0.6))
            tg = np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(420, 700)])
            Re = Rg @ random_rotation(rng, rng.uniform(0, 0.12))
            te = tg + rng.normal(size=3) * [6.0, 6.0, 20.0]
            rows.append((o, im, Re.astype(F), te.astype(F), Rg.astype(F), tg.astype(F)))
            z, _ = depth32(objs[o]["vertices"], objs[o]["faces"], pose(rows[-1][4], rows[-1][5]), CAMS[im], H, W)
            hit = z > 0
            if j % 4 >= 2 and hit.any():                          # an occluder over the left half of the instance
                xs = np.where(hit.any(axis=0))[0]
                left = hit & (np.arange(W)[None, :] <= (xs.min() + xs.max()) // 2)
                z = np.where(left, z - F(60.0), z)
            depth[im] = np.where(hit, np.minimum(depth[im], np.where(hit, z, np.inf)), depth[im])
    depth[:, 10:20, 30:50] = 0.0                                  # missing
    raw = np.rint(depth.astype(np.float64) / 0.5).astype(np.uint16)
    return {"objects": objs, "obj_ids": np.array([r[0] for r in rows]), "image_index": np.array([r[1] for r in rows], dtype=np.int32),
            "R_est": np.stack([r[2] for r in rows]), "t_est": np.stack([r[3] for r in rows]), "R_gt": np.stack([r[4] for r in rows]),
            "t_gt": np.stack([r[5] for r in rows]), "depth_u16": raw, "depth_scale": 0.5, "K": k33(CAMS)}


def k33(cams):
    K = np.zeros((len(cams), 3, 3), dtype=F)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = cams[:, 0], cams[:, 1], cams[:, 2], cams[:, 3], 1
    return K


def depth_mm32(raw, depth_scale):
    """What pp_depth_u16_scaled writes for s = f32(1000 depth_scale): (f32(d) * s) / 1000 in float32."""
    return (raw.astype(F) * F(depth_scale * 1000.0)) / F(1000)


def reference(scene, delta=15.0, taus=TAUS, near=1.0):
    """The oracle's answer for a scene dict (as mixed_scene returns): every distinct (image, object, pose) rendered once on the full
    frame (a non-finite pose: nothing) -> {"counts" (P, 2 + T), "vsd" (P, T) float32, "counts64", "vsd64", "fragile" (P, 2 + T),
    "n_views", "near_count", "z_est", "z_gt" lists, "depth_mm"}."""
    objs = scene["objects"]
    dm = scene["depth_mm"] if "depth_mm" in scene else depth_mm32(scene["depth_u16"], scene["depth_scale"])
    K = np.asarray(scene["K"])
    K = np.broadcast_to(K, (len(dm), 3, 3)) if K.ndim == 2 else K
    cache, near_total = {}, 0
    out = {k: [] for k in ("counts", "vsd", "counts64", "vsd64", "fragile", "z_est", "z_gt")}
    for p, o in enumerate(scene["obj_ids"].tolist()):
        im = int(scene["image_index"][p])
        K4 = (K[im][0, 0], K[im][1, 1], K[im][0, 2], K[im][1, 2])
        z = []
        for R, t in ((scene["R_est"][p], scene["t_est"][p]), (scene["R_gt"][p], scene["t_gt"][p])):
            P4 = pose(R, t)
            key = (im, o, P4.tobytes())
            if key not in cache:
                win = None if np.all(np.isfinite(P4)) else (0, 0, 0, 0)
                cache[key], nc = depth32(objs[o]["vertices"], objs[o]["faces"], P4, K4, H if "hw" not in scene else scene["hw"][0],
                                         W if "hw" not in scene else scene["hw"][1], near, win)
                near_total += nc
            z.append(cache[key])
        d = objs[o]["info"]["diameter"]
        c32, e32 = vsd32(z[0], z[1], dm[im], K4, d, delta, taus)
        c64, e64 = vsd64(z[0], z[1], dm[im], K4, d, delta, taus)
        for k, v in zip(out, (c32, e32, c64, e64, fragile(z[0], z[1], dm[im], K4, d, delta, taus), z[0], z[1])):
            out[k].append(v)
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(n_views=len(cache), near_count=near_total, depth_mm=dm)
    return res
