"""Numpy statement of the pose-verification contract of include/picopose_hip.h ("POSE VERIFICATION"), written from that text and
built on vsd_oracle.depth32: the eight counters in float32 in the stated operation order (counts32), the same counters from float64
definitions (counts64), a dense decoder of COCO RLE to the column-major mask (decode) with the inverse used to make test masks
(rle), the score formulas (scores) and a whole call (reference).  It is checked against closed forms in
tests/test_pose_verify_cpu.py; the kernels are held to it, bit for bit, in tests/test_pose_verify_gpu.py."""
import numpy as np

import vsd_oracle as vo

F = np.float32
NAMES = ("render", "inter", "valid", "agree", "front", "behind", "vis", "vis_inter")


def decode(segmentation):
    """{"size": [H, W], "counts": [run lengths]} (uncompressed COCO RLE: column-major runs, zeros first) -> (H, W) bool."""
    h, w = (int(v) for v in segmentation["size"])
    counts = np.asarray(segmentation["counts"], dtype=np.int64)
    assert counts.min() >= 0 and counts.sum() == h * w
    flat = np.repeat(np.arange(len(counts)) % 2, counts).astype(bool)      # pixel x * H + y
    return flat.reshape(w, h).T


def rle(mask):
    """(H, W) bool -> the uncompressed COCO RLE of it (written here, independent of the package's encoder)."""
    m = np.asarray(mask, dtype=bool)
    flat = m.T.reshape(-1)
    counts, cur, run = [], False, 0
    for v in flat.tolist():
        if v == cur:
            run += 1
        else:
            counts.append(run)
            cur, run = v, 1
    counts.append(run)
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": counts}


def counts32(z, mask, z_test, K4, delta):
    """One view: its render z (H, W) float32 (0 = nothing), its mask (H, W) bool, the test depth (H, W) float32 or None -> (8,) int64
    in float32, operation for operation: xr = (f32(x) - cx) / fx, r = sqrt((xr xr + yr yr) + 1), d = z r, d_test = z_test r,
    e = d - d_test."""
    z = np.asarray(z, dtype=F)
    cover, m = z > 0, np.asarray(mask, dtype=bool)
    if z_test is None:
        n, i = int(cover.sum()), int((cover & m).sum())
        return np.array([n, i, 0, 0, 0, 0, n, i], dtype=np.int64)
    zt = np.asarray(z_test, dtype=F)
    r = vo._rays32(K4, *z.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = cover & (zt > 0)                                    # (a NaN is missing)
        e = z * r - zt * r
        front, behind = valid & (e > F(delta)), valid & (-e > F(delta))
    agree, vis = valid & ~front & ~behind, cover & ~front
    return np.array([x.sum() for x in (cover, cover & m, valid, agree, front, behind, vis, vis & m)], dtype=np.int64)


def counts64(z, mask, z_test, K4, delta):
    """The same counters from the definition in float64 (the float32 depths and camera the kernel is given, delta as its float32)."""
    z = np.asarray(z, dtype=np.float64)
    cover, m = z > 0, np.asarray(mask, dtype=bool)
    if z_test is None:
        n, i = int(cover.sum()), int((cover & m).sum())
        return np.array([n, i, 0, 0, 0, 0, n, i], dtype=np.int64)
    fx, fy, cx, cy = (float(F(k)) for k in K4)
    H, W = z.shape
    xr, yr = (np.arange(W, dtype=np.float64)[None, :] - cx) / fx, (np.arange(H, dtype=np.float64)[:, None] - cy) / fy
    r = np.sqrt(xr * xr + yr * yr + 1.0)
    zt = np.asarray(z_test, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        valid = cover & (zt > 0)
        e = np.where(valid, z * r - np.where(valid, zt, 0.0) * r, 0.0)
    front, behind = valid & (e > float(F(delta))), valid & (-e > float(F(delta)))
    agree, vis = valid & ~front & ~behind, cover & ~front
    return np.array([x.sum() for x in (cover, cover & m, valid, agree, front, behind, vis, vis & m)], dtype=np.int64)


def scores(counts, area, with_depth):
    """counts (P, 8), area (P,) -> (iou, visible_iou, agreement, score), float64, from the integers alone; a zero denominator gives
    0 for the two ious and 1 for the agreement."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 8)
    a = np.asarray(area, dtype=np.int64).reshape(-1)
    out = []
    for num, den, empty in ((c[:, 1], c[:, 0] + a - c[:, 1], 0.0), (c[:, 7], c[:, 6] + a - c[:, 7], 0.0), (c[:, 3], c[:, 3] + c[:, 5], 1.0)):
        out.append(np.array([float(n) / float(d) if d > 0 else empty for n, d in zip(num.tolist(), den.tolist())], dtype=np.float64))
    return out[0], out[1], out[2], (out[1] * out[2] if with_depth else out[0])


def render(objs, obj_id, pose, K4, H, W, near=1.0):
    """The full-frame render of one view; a pose with a NaN or an infinity renders nothing -> ((H, W) float32, near drops)."""
    P = np.asarray(pose, dtype=F)
    if not np.all(np.isfinite(P[:3])):
        return np.zeros((H, W), dtype=F), 0
    o = objs[int(obj_id)]
    return vo.depth32(o["vertices"], o["faces"], P, K4, H, W, near)


def reference(objs, obj_ids, poses, image_index, cams, H, W, masks, mask_index, depth=None, delta=15.0):
    """A whole call: P views, masks a list of (H, W) bool, depth (n_images, H, W) float32 mm or None -> {"counts", "counts64" (P, 8),
    "mask_area" (M,), "near" (P,), "z" the renders}."""
    out = {"counts": [], "counts64": [], "near": [], "z": []}
    for v in range(len(obj_ids)):
        i = int(image_index[v])
        z, n = render(objs, obj_ids[v], poses[v], cams[i], H, W)
        zt = None if depth is None else np.asarray(depth[i], dtype=F)
        out["counts"].append(counts32(z, masks[int(mask_index[v])], zt, cams[i], delta))
        out["counts64"].append(counts64(z, masks[int(mask_index[v])], zt, cams[i], delta))
        out["near"].append(n)
        out["z"].append(z)
    res = {k: np.array(v).reshape((len(obj_ids),) + ((8,) if k.startswith("counts") else ())) for k, v in out.items() if k != "z"}
    res.update(z=out["z"], mask_area=np.array([int(np.asarray(m).sum()) for m in masks], dtype=np.int64))
    return res
