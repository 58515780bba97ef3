"""Numpy statement of the scene-ground-truth contract of include/picopose_hip.h ("SCENE GROUND TRUTH"), written from that text and
built on vsd_oracle.depth32 with the canvas camera: the padded render (render), the float32 counts, boxes and masks (info32), the
float64 definition of the counts (counts64), the composite of an image's views (composite) and a whole call (reference).  It is
checked against fixed answers in tests/test_scene_gt_cpu.py; the kernels are held to it in tests/test_scene_gt_gpu.py."""
import numpy as np

import vsd_oracle as vo

F = np.float32
EMPTY = (0, 0, -1, -1)


def pad_of(pad, H, W):
    return (W, H) if isinstance(pad, str) else (int(pad[0]), int(pad[1]))


def canvas_k4(K4, pad):
    """(fx, fy, f32(cx + pad_x), f32(cy + pad_y)): the sums in float32, rounded once."""
    fx, fy, cx, cy = (F(k) for k in K4)
    return (fx, fy, F(cx + F(pad[0])), F(cy + F(pad[1])))


def render(vertices, faces, pose, K4, H, W, pad, near=1.0):
    """The view on the canvas of (H + 2 pad_y) x (W + 2 pad_x) samples -> ((Hc, Wc) float32 Z, triangles dropped at the near plane).
    A pose with a NaN or an infinity renders nothing."""
    Hc, Wc = H + 2 * pad[1], W + 2 * pad[0]
    P = np.asarray(pose, dtype=F)
    if not np.all(np.isfinite(P[:3])):
        return np.zeros((Hc, Wc), dtype=F), 0
    return vo.depth32(vertices, faces, P, canvas_k4(K4, pad), Hc, Wc, near)


def box(mask, pad=(0, 0)):
    """Inclusive corners {x_min, y_min, x_max, y_max} of a mask, moved from canvas to frame coordinates; empty: {0, 0, -1, -1}."""
    ys, xs = np.where(mask)
    if len(xs) == 0:
        return EMPTY
    return (int(xs.min()) - pad[0], int(ys.min()) - pad[1], int(xs.max()) - pad[0], int(ys.max()) - pad[1])


def visible32(z, z_test, K4, delta):
    """visib_gt of the VSD contract in float32, operation for operation, on frame-sized images."""
    z, z_test = np.asarray(z, dtype=F), np.asarray(z_test, dtype=F)
    r = vo._rays32(K4, *z.shape)
    with np.errstate(invalid="ignore"):
        missing = ~(z_test > 0)
        d, d_test = z * r, z_test * r
        return (d > 0) & (missing | (d - d_test <= F(delta)))


def visible64(z, z_test, K4, delta):
    """The same in float64 from the float32 depths (delta as the float32 number the kernel is given)."""
    fx, fy, cx, cy = (float(F(k)) for k in K4)
    H, W = z.shape
    xr, yr = (np.arange(W, dtype=np.float64)[None, :] - cx) / fx, (np.arange(H, dtype=np.float64)[:, None] - cy) / fy
    r = np.sqrt(xr * xr + yr * yr + 1.0)
    zt = np.asarray(z_test, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        missing = ~(zt > 0)
    d, d_test = np.asarray(z, dtype=np.float64) * r, np.where(missing, 0.0, zt) * r
    return (d > 0) & (missing | (d - d_test <= float(F(delta))))


def info32(zc, z_test, K4, H, W, pad, delta=15.0):
    """Per view from its canvas render and the test depth of its image (frame-sized float32 mm) -> {"all", "inframe", "valid", "visib",
    "bbox_obj", "bbox_visib", "mask_all", "mask_visib" ((H, W) uint8 0 / 255)}."""
    zf = zc[pad[1]:pad[1] + H, pad[0]:pad[0] + W]
    with np.errstate(invalid="ignore"):
        present = np.asarray(z_test, dtype=F) > 0
    vis = visible32(zf, z_test, K4, delta)
    return {"all": int((zc > 0).sum()), "inframe": int((zf > 0).sum()), "valid": int(((zf > 0) & present).sum()), "visib": int(vis.sum()),
            "bbox_obj": box(zc > 0, pad), "bbox_visib": box(vis), "mask_all": ((zf > 0) * 255).astype(np.uint8),
            "mask_visib": (vis * 255).astype(np.uint8)}


def counts64(zc, z_test, K4, H, W, pad, delta=15.0):
    """{all, valid, visib} by the float64 definition."""
    zf = zc[pad[1]:pad[1] + H, pad[0]:pad[0] + W]
    with np.errstate(invalid="ignore"):
        present = np.asarray(z_test, dtype=np.float64) > 0
    return (int((zc > 0).sum()), int(((zf > 0) & present).sum()), int(visible64(zf, z_test, K4, delta).sum()))


def composite(frames, labels=None):
    """The views of ONE image (frame-sized float32 Z, in call order) -> (scene_depth (H, W) float32, instance_map (H, W) int32): per
    pixel the minimum of (bits of Z) << 32 | k over the covering views; the map holds labels[k] (k itself without labels), -1 = background."""
    H, W = frames[0].shape
    word = np.full((H, W), ~np.uint64(0), dtype=np.uint64)
    for k, z in enumerate(frames):
        key = (np.ascontiguousarray(z, dtype=F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(k)
        word = np.where(z > 0, np.minimum(word, key), word)
    hit = word != ~np.uint64(0)
    depth = np.where(hit, (word >> np.uint64(32)).astype(np.uint32).view(F), F(0)).astype(F)
    k = (word & np.uint64(0xFFFFFFFF)).astype(np.int64)
    lab = np.arange(len(frames)) if labels is None else np.asarray(labels)
    return depth, np.where(hit, lab[np.where(hit, k, 0)], -1).astype(np.int32)


def reference(objs, obj_ids, poses, image_index, cams, H, W, pad="bop", depth=None, delta=15.0, near=1.0):
    """A whole call: U views (objs[obj_ids[v]] under poses[v] (4, 4) in image image_index[v]), cams (n_images, 4), depth
    (n_images, H, W) float32 mm or None (composite visibility) -> {"counts" (U, 3) = all, valid, visib, "inframe" (U,), "counts64"
    (U, 3), "bbox_obj", "bbox_visib" (U, 4), "mask_all", "mask_visib" (U, H, W), "near" (U,), "scene_depth", "instance_map"
    (n_images, H, W), "z" the canvas renders, "fragile" (U,): the pixels float32 may decide differently from float64}."""
    pad = pad_of(pad, H, W)
    U, n_images = len(obj_ids), len(cams)
    z, near_n = [], []
    for v in range(U):
        o = objs[int(obj_ids[v])]
        zc, n = render(o["vertices"], o["faces"], poses[v], cams[image_index[v]], H, W, pad, near)
        z.append(zc)
        near_n.append(n)
    frames = [zc[pad[1]:pad[1] + H, pad[0]:pad[0] + W] for zc in z]
    scene_depth, inst = np.zeros((n_images, H, W), dtype=F), np.full((n_images, H, W), -1, dtype=np.int32)
    for i in range(n_images):
        views = [v for v in range(U) if image_index[v] == i]
        if views:
            scene_depth[i], inst[i] = composite([frames[v] for v in views], views)
    test = scene_depth if depth is None else np.asarray(depth, dtype=F)
    out = {k: [] for k in ("counts", "inframe", "counts64", "bbox_obj", "bbox_visib", "mask_all", "mask_visib", "fragile")}
    for v in range(U):
        i = int(image_index[v])
        r = info32(z[v], test[i], cams[i], H, W, pad, delta)
        out["counts"].append((r["all"], r["valid"], r["visib"]))
        out["inframe"].append(r["inframe"])
        out["counts64"].append(counts64(z[v], test[i], cams[i], H, W, pad, delta))
        for k in ("bbox_obj", "bbox_visib", "mask_all", "mask_visib"):
            out[k].append(r[k])
        out["fragile"].append(int(vo.fragile(frames[v], frames[v], test[i], cams[i], 1.0, delta)[0]))
    res = {k: np.array(v) for k, v in out.items()}
    res.update(near=np.array(near_n), scene_depth=scene_depth, instance_map=inst, z=z)
    return res


# ---- the scenes of the tests ---------------------------------------------------------------------------------------------------------
def edge_scene():
    """CAMS[0], 90 x 120: four instances over the frame's borders, the camera inside the sphere (a whole-canvas window, near-plane
    drops), a plate off the frame but on the canvas, a cube behind the camera, an instance over the missing block and an occluded one."""
    objs = vo.objects()
    I, rot = np.eye(3), vo.random_rotation(np.random.default_rng(1))
    rows = [(1, rot, (-280.0, 0, 500)), (1, rot, (290.0, 0, 500)), (1, rot, (0.0, -215, 500)), (2, I, (300.0, 225, 500)), (2, I, (0.0, 0, 40)),
            (3, I, (-330.0, 0, 500)), (1, rot, (0.0, 0, -500)), (2, I, (20.0, 10, 520)), (1, rot, (0.0, 0, 600))]
    depth = np.full((1, vo.H, vo.W), 560.0, dtype=F)
    depth[0, 40:50, 55:70] = 0.0
    depth[0, :, :8] = 300.0
    return {"objects": objs, "obj_ids": np.array([r[0] for r in rows]), "image_index": np.zeros(len(rows), dtype=np.int32),
            "R": np.stack([F(r[1]) for r in rows]), "t": np.stack([F(r[2]) for r in rows]), "depth": depth, "cams": vo.CAMS[:1]}


def plate_scene(ts):
    p = vo.plate(vo.PLATE_N)
    return {"objects": {3: {"vertices": p["vertices"], "faces": p["faces"], "info": {"diameter": vo.PLATE_DIAMETER}}},
            "obj_ids": np.full(len(ts), 3), "image_index": np.zeros(len(ts), dtype=np.int32), "R": np.stack([np.eye(3, dtype=F)] * len(ts)),
            "t": np.array(ts, dtype=F), "cams": np.array([vo.PLATE_K4], dtype=F)}


def poses_of(scene):
    return [vo.pose(R, t) for R, t in zip(scene["R"], scene["t"])]


def scene_reference(scene, H, W, pad="bop", depth="scene", delta=15.0):
    d = scene.get("depth") if isinstance(depth, str) else depth
    return reference(scene["objects"], scene["obj_ids"], poses_of(scene), scene["image_index"], scene["cams"], H, W, pad, d, delta)
