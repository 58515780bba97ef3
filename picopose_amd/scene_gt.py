"""Scene ground truth on the GPU: what BOP's scene_gt_info.json, mask and mask_visib hold, from scene_gt.json, the models and
(optionally) the test depth images — the per-instance pixel counts, visible fraction, boxes and masks (scene_gt_info), the files'
schema (format_gt_info, dataset_gt_info), BOP19 targets (targets_from_gt_info) and CNOS-shaped detection records of the ground
truth (gt_detections, with masks.rle_from_mask).

The contract is "SCENE GROUND TRUTH" of include/picopose_hip.h (csrc/pp_scene_gt.hip; tests/scene_gt_oracle.py restates it in numpy).
It is the BOP toolkit's calc_gt_info / calc_gt_masks written from memory: the toolkit cannot be run next to this library, parity
with its pixels is UNPINNED, and the header lists the known differences (sampling convention, near-plane rule, box convention).
The planners (windows, view groups, depth conversion, cameras) and the packing of a call's tables are scene.py's."""
import math

import numpy as np
import torch

from . import _lib
from . import scene as scn
from .masks import rle_from_mask
from .scene import DEFAULT_WORKSPACE_BYTES

MASKS = (None, "visib", "all", "both")


def _pad(pad, H, W):
    """pad -> (pad_x, pad_y): "bop" is the toolkit's canvas as remembered, (W, H); otherwise two non-negative ints."""
    if isinstance(pad, str):
        if pad != "bop":
            raise ValueError(f"pad must be 'bop' or (pad_x, pad_y), got {pad!r}")
        return W, H
    try:
        px, py = pad
    except (TypeError, ValueError):
        raise ValueError(f"pad must be 'bop' or (pad_x, pad_y), got {pad!r}") from None
    if not all(isinstance(p, (int, np.integer)) and not isinstance(p, bool) and p >= 0 for p in (px, py)):
        raise ValueError(f"pad must hold two non-negative ints, got {pad!r}")
    return int(px), int(py)


def canvas_cams(cams, pad_x, pad_y):
    """(n, 4) float32 frame cameras -> the canvas cameras (fx, fy, f32(cx + pad_x), f32(cy + pad_y)): float32 sums, rounded once."""
    out = np.array(cams, dtype=np.float32)
    out[:, 2] = out[:, 2] + np.float32(pad_x)
    out[:, 3] = out[:, 3] + np.float32(pad_y)
    return out


def image_groups(cost, view_img, frame_bytes, workspace_bytes):
    """Groups of WHOLE images for a composite call.  cost (U,): the bytes of each view (8 per window sample and per triangle, + 256);
    view_img (U,) ascending; frame_bytes = 8 H W, the composite's words of one image.  A group is a range of images [i0, i1) (images
    without views inside it included: they cost their words) whose views and words fit `workspace_bytes` less the three 256-byte
    roundings of the layout.  -> [(v0, v1, i0, i1)]: views [v0, v1) of the sorted order.  ValueError when one image alone does not fit."""
    budget = max(int(workspace_bytes) - 768, 0)
    groups, U = [], len(view_img)
    v = 0
    cur = None                                                    # [v0, i0, bytes of the views]
    while v < U:
        i = int(view_img[v])
        e = v
        while e < U and view_img[e] == i:
            e += 1
        c = int(cost[v:e].sum())
        if c + frame_bytes > budget:
            raise ValueError(f"the {e - v} views of image {i} need {c + frame_bytes + 768} bytes with the composite: more than "
                             f"workspace_bytes = {workspace_bytes}")
        if cur is not None and cur[2] + c + (i + 1 - cur[1]) * frame_bytes > budget:
            groups.append((cur[0], v, cur[1], int(view_img[v - 1]) + 1))
            cur = None
        if cur is None:
            cur = [v, i, 0]
        cur[2] += c
        v = e
    if cur is not None:
        groups.append((cur[0], U, cur[1], int(view_img[U - 1]) + 1))
    return groups


def scene_gt_info(models, obj_ids, R, t, K, depth=None, resolution=None, image_index=None, depth_scale=None, delta=15.0, pad="bop",
                  near=1.0, window="auto", masks=None, composite=False, workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """The ground-truth info of U (object, pose) views over n_images frames ->
      {"px_count_all", "px_count_valid", "px_count_visib": (U,) int32, "bbox_obj", "bbox_visib": (U, 4) int32 INCLUSIVE corners
       {x_min, y_min, x_max, y_max} in frame coordinates (bbox_obj may leave the frame; empty: {0, 0, -1, -1}), "near_counts" (U,) int32
       — device tensors; "visib_fract": (U,) float64 numpy = px_count_visib / px_count_all, 0 where nothing is covered;
       "near_count": the triangles dropped at the near plane, "n_groups": the pp_scene_gt calls made;
       with masks: "mask_visib" and / or "mask_all" (U, H, W) uint8 0 / 255 device tensors;
       with composite=True: "scene_depth" (n_images, H, W) float32 (0 = background) and "instance_map" (n_images, H, W) int32, the
       index in THIS call's obj_ids of the nearest view (the lower index on equal depth), -1 = background}.

    depth: (n_images, H, W) uint16 raw with `depth_scale` or float millimetres, as evaluation.vsd_errors takes it; a value that is not
    > 0 is missing, and a covered pixel with a missing depth is visible.  depth=None selects COMPOSITE visibility: `resolution` =
    (H, W) is then required and the test depth of an image is the composite of the views given for it, so an instance is hidden by
    the other instances alone (delta = 0: exact mutual occlusion).  K (3, 3) or (n_images, 3, 3), image_index (U,) as render_depth.
    pad: "bop" renders on the toolkit's canvas as remembered, (pad_x, pad_y) = (W, H), so that px_count_all and bbox_obj see the object
    past the frame; (0, 0) renders the frame only.  masks: None, "visib", "all" or "both".  window and near as render_depth.
    The views are processed in as many calls as `workspace_bytes` needs, with identical results; when the composite runs (depth is
    None or composite=True) a call holds whole images, and ValueError is raised when one image's views alone exceed the bound.
    A pose with a NaN or an infinity renders nothing: zero counts, empty boxes.  U = 0: empty tensors, no launch.
    ValueError as vsd_errors, and for pad, delta (negative or not finite), masks, composite, a missing or mismatching resolution."""
    obj = scn.obj_index(models, obj_ids)
    U, dev = len(obj), models.device
    scn.check_scalars(near, window, workspace_bytes)
    if not (isinstance(delta, (int, float)) and not isinstance(delta, bool) and math.isfinite(delta) and delta >= 0):
        raise ValueError(f"delta must be a non-negative number, got {delta!r}")
    if masks not in MASKS:
        raise ValueError(f"masks must be one of {MASKS}, got {masks!r}")
    if not isinstance(composite, (bool, np.bool_)):
        raise ValueError(f"composite must be a bool, got {composite!r}")
    res = None
    if resolution is not None:
        res = scn.resolution_hw(resolution)
        if res is None or not scn.frame_in_range(*res):
            raise ValueError(f"resolution must be (H, W), positive with H W < 2^31, got {resolution!r}")
    if depth is None:
        if res is None:
            raise ValueError("depth=None selects composite visibility: resolution=(H, W) is required")
        if depth_scale is not None:
            raise ValueError("depth_scale without depth")
        H, W = res
        n_images, scale = scn.n_images_of(K), None
    else:
        n_images, H, W, scale = scn.check_depth(depth, depth_scale)
        if res is not None and res != (H, W):
            raise ValueError(f"resolution {res} is not the depth images' {(H, W)}")
    pad_x, pad_y = _pad(pad, H, W)
    Hc, Wc = H + 2 * pad_y, W + 2 * pad_x
    if Hc * Wc >= 2 ** 31:
        raise ValueError(f"the padded canvas {Hc} x {Wc} must hold fewer than 2^31 samples")
    Rh, th = scn.host_f32("R", R, U, (3, 3)), scn.host_f32("t", t, U, (3,))
    cams = scn.cameras(K, n_images)
    img = scn.image_index(image_index, U, n_images)
    want_all, want_visib = masks in ("all", "both"), masks in ("visib", "both")
    run_composite = bool(composite) or depth is None

    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)       # noqa: E731
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)        # noqa: E731
    if U == 0:
        out = {"px_count_all": i32(0), "px_count_valid": i32(0), "px_count_visib": i32(0), "bbox_obj": i32(0, 4), "bbox_visib": i32(0, 4),
               "near_counts": i32(0), "visib_fract": np.zeros(0, dtype=np.float64), "near_count": 0, "n_groups": 0}
        if want_all:
            out["mask_all"] = u8(0, H, W)
        if want_visib:
            out["mask_visib"] = u8(0, H, W)
        if composite:
            out["scene_depth"] = torch.zeros((n_images, H, W), dtype=torch.float32, device=dev)
            out["instance_map"] = torch.full((n_images, H, W), -1, dtype=torch.int32, device=dev)
        return out

    ccams = canvas_cams(cams, pad_x, pad_y)
    if not np.all(np.isfinite(ccams)):
        raise ValueError("K plus the pad is not finite in float32")
    poses = scn.pose44(Rh, th)
    windows = scn.view_windows(models, obj, img, poses, ccams, Hc, Wc, near, window)
    # the order of the calls: as given, or (composite) stably by image, so that a call holds whole images
    if run_composite:
        order = np.argsort(img, kind="stable")
        groups = image_groups(scn.view_cost(models, obj[order], windows[order]), img[order], 8 * H * W, workspace_bytes)
    else:
        order = np.arange(U)
        groups = [(int(g[0][0]), int(g[0][-1]) + 1, 0, n_images) for g in scn.view_groups(models, obj, windows, None, None, workspace_bytes)]
    scn.require_gpu(dev)
    depth_d = None if depth is None else scn.depth_mm(depth, scale, dev)
    s_obj, s_img, s_pose, s_win = obj[order], img[order], poses[order], windows[order]
    counts, boxes, near_d = i32(U, 3), i32(U, 8), i32(U)
    m_all = u8(U, H, W) if want_all else None
    m_vis = u8(U, H, W) if want_visib else None
    scene_depth = torch.zeros((n_images, H, W), dtype=torch.float32, device=dev) if composite else None
    inst_map = torch.full((n_images, H, W), -1, dtype=torch.int32, device=dev) if composite else None
    at = lambda a, n: None if a is None else a[n:]      # noqa: E731  (an optional output from its row n on)
    for v0, v1, i0, i1 in groups:
        packed = scn.PackedScene(models, cams[i0:i1], H, W, near, s_obj[v0:v1], s_img[v0:v1] - i0, s_pose[v0:v1], s_win[v0:v1])
        ccam = np.ascontiguousarray(ccams[i0:i1])
        need = _lib.workspace_bytes("pp_scene_gt_workspace_bytes", packed.samples, packed.faces, (i1 - i0) * H * W if run_composite else 0)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        label_d, ccam_d = torch.from_numpy(order[v0:v1].astype(np.int32)).to(dev), torch.from_numpy(ccam).to(dev)
        _lib.call("pp_scene_gt", packed.scene, ccam_d, ccam, pad_x, pad_y, at(depth_d, i0), float(delta), label_d, 1, ws, ws.numel(),
                  counts[v0:], boxes[v0:], near_d[v0:], at(m_all, v0), at(m_vis, v0), at(scene_depth, i0), at(inst_map, i0))
    if run_composite and not np.array_equal(order, np.arange(U)):  # back to the caller's order
        inv = torch.from_numpy(np.argsort(order, kind="stable")).to(dev)
        counts, boxes, near_d = counts[inv], boxes[inv], near_d[inv]
        m_all = None if m_all is None else m_all[inv]
        m_vis = None if m_vis is None else m_vis[inv]
    c = counts.cpu().numpy().astype(np.float64)
    out = {"px_count_all": counts[:, 0], "px_count_valid": counts[:, 1], "px_count_visib": counts[:, 2], "bbox_obj": boxes[:, :4],
           "bbox_visib": boxes[:, 4:], "near_counts": near_d,
           "visib_fract": np.divide(c[:, 2], c[:, 0], out=np.zeros(U, dtype=np.float64), where=c[:, 0] > 0),
           "near_count": int(near_d.sum().item()), "n_groups": len(groups)}
    if want_all:
        out["mask_all"] = m_all
    if want_visib:
        out["mask_visib"] = m_vis
    if composite:
        out["scene_depth"], out["instance_map"] = scene_depth, inst_map
    return out


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _xywh(box):
    """Inclusive corners -> the file's [x_min, y_min, x_max - x_min, y_max - y_min]; an empty box -> [-1, -1, -1, -1]."""
    x0, y0, x1, y1 = (int(v) for v in box)
    return [-1, -1, -1, -1] if x1 < x0 or y1 < y0 else [x0, y0, x1 - x0, y1 - y0]


def format_gt_info(result):
    """scene_gt_info's result -> a list of dicts in scene_gt_info.json's per-instance schema: bbox_obj, bbox_visib, px_count_all,
    px_count_valid, px_count_visib, visib_fract.  A box is [x_min, y_min, x_max - x_min, y_max - y_min] — the toolkit's calc_2d_bbox
    AS REMEMBERED (parity unpinned: width = max - min, not the pixel count) — and an empty box is [-1, -1, -1, -1]."""
    bo, bv = _np(result["bbox_obj"]), _np(result["bbox_visib"])
    na, nv, ns = _np(result["px_count_all"]), _np(result["px_count_valid"]), _np(result["px_count_visib"])
    fr = np.asarray(result["visib_fract"], dtype=np.float64)
    return [{"bbox_obj": _xywh(bo[k]), "bbox_visib": _xywh(bv[k]), "px_count_all": int(na[k]), "px_count_valid": int(nv[k]),
             "px_count_visib": int(ns[k]), "visib_fract": float(fr[k])} for k in range(len(fr))]


def dataset_gt_batches(ground_truth, cameras, models, resolution, depth_images=None, images_per_call=64, **kw):
    """The batching of `dataset_gt_info`: one scene_gt_info call (kw goes to it) per `images_per_call` images -> yields (batch, obj,
    result): batch = the [(scene_id, im_id)] of the call, obj = the object ids of each image's instances (one array per image), result =
    scene_gt_info's for the concatenated instances, image after image."""
    if not (isinstance(images_per_call, int) and images_per_call > 0):
        raise ValueError(f"images_per_call must be a positive int, got {images_per_call!r}")
    images = [(int(s), int(im)) for s, per in ground_truth.items() for im in per]
    for b0 in range(0, len(images), images_per_call):
        batch = images[b0:b0 + images_per_call]
        obj, R, t, idx, Kb = [], [], [], [], []
        for j, (s, im) in enumerate(batch):
            gt = ground_truth[s][im]
            if s not in cameras or im not in cameras[s]:
                raise ValueError(f"cameras holds no entry for scene {s}, image {im}")
            Kb.append(np.asarray(cameras[s][im]["K"], dtype=np.float64).reshape(3, 3))
            obj.append(np.asarray(gt["obj_id"], dtype=np.int64))
            R.append(np.asarray(gt["R"], dtype=np.float64).reshape(-1, 3, 3))
            t.append(np.asarray(gt["t"], dtype=np.float64).reshape(-1, 3))
            idx.append(np.full(len(gt["obj_id"]), j, dtype=np.int32))
        depth, depth_scale = None, None
        if depth_images is not None:
            frames = [np.asarray(depth_images(*k) if callable(depth_images) else depth_images[k[0]][k[1]]) for k in batch]
            if any(f.ndim != 2 or f.shape != frames[0].shape for f in frames):
                raise ValueError("depth images of one call must share one (H, W) resolution")
            scale = np.array([cameras[k[0]][k[1]]["depth_scale"] for k in batch], dtype=np.float64)
            if all(f.dtype == np.uint16 for f in frames):
                depth, depth_scale = np.stack(frames), scale
            else:
                depth = np.stack([f.astype(np.float32) * np.float32(sc) for f, sc in zip(frames, scale)])
        yield batch, obj, scene_gt_info(models, np.concatenate(obj), np.concatenate(R), np.concatenate(t), np.stack(Kb), depth=depth,
                                        resolution=resolution, image_index=np.concatenate(idx), depth_scale=depth_scale, **kw)


def dataset_gt_info(ground_truth, cameras, models, resolution, depth_images=None, images_per_call=64, **kw):
    """scene_gt_info.json for whole scenes.  ground_truth / cameras: {scene_id: read_scene_gt(...) / read_scene_camera(...)} and
    depth_images as evaluation.match_and_score takes them ({scene_id: {im_id: (H, W) array}} or a callable (scene_id, im_id) -> array;
    raw values scaled by the camera's depth_scale; None: composite visibility).  One scene_gt_info call per `images_per_call` images
    (kw goes to it) -> {scene_id: {im_id: [info dicts in instance order]}} (format_gt_info's dicts)."""
    out = {int(s): {} for s in ground_truth}
    for batch, obj, r in dataset_gt_batches(ground_truth, cameras, models, resolution, depth_images, images_per_call, **kw):
        info, k = format_gt_info(r), 0
        for (s, im), o in zip(batch, obj):
            out[s][im] = info[k:k + len(o)]
            k += len(o)
    return out


def targets_from_gt_info(ground_truth, gt_info, min_visib_fract=0.1):
    """BOP19 targets from ground truth and its info -> (N, 4) int64 rows {scene_id, im_id, obj_id, inst_count} (what
    evaluation.read_targets returns), sorted by (scene, image, object): inst_count = the instances of the object in the image with
    visib_fract >= min_visib_fract; rows with count 0 are left out.  This is the BOP19 rule AS REMEMBERED (parity unpinned)."""
    rows = {}
    for s, per in ground_truth.items():
        for im, gt in per.items():
            info = gt_info[int(s)][int(im)]
            if len(info) != len(gt["obj_id"]):
                raise ValueError(f"scene {s}, image {im}: {len(info)} info entries for {len(gt['obj_id'])} instances")
            for o, e in zip(np.asarray(gt["obj_id"]).tolist(), info):
                if e["visib_fract"] >= min_visib_fract:
                    key = (int(s), int(im), int(o))
                    rows[key] = rows.get(key, 0) + 1
    return np.array([k + (n,) for k, n in sorted(rows.items())], dtype=np.int64).reshape(-1, 4)


def gt_detections(obj_ids, result, scene_id, im_id, score=1.0, time=0.0):
    """CNOS-shaped detection records of one image's ground truth, for running the estimator on ground-truth masks:
    obj_ids (U,) and result = scene_gt_info(..., masks="visib" or "both") of that image's instances -> a list of
    {"scene_id", "image_id", "category_id", "bbox" [x, y, w, h] of the visible mask (w, h pixel counts), "score", "time",
    "segmentation": rle_from_mask(mask_visib)} for the instances with a non-empty visible mask, in instance order.
    provider.test_batch.assemble_test_image and pipeline.infer_detections accept the records as they are."""
    if "mask_visib" not in result:
        raise ValueError("gt_detections needs scene_gt_info(..., masks='visib' or 'both')")
    ids = np.asarray(obj_ids.cpu() if isinstance(obj_ids, torch.Tensor) else obj_ids).reshape(-1)
    masks, boxes, n = _np(result["mask_visib"]), _np(result["bbox_visib"]), _np(result["px_count_visib"])
    if len(ids) != len(masks):
        raise ValueError(f"{len(ids)} obj_ids for {len(masks)} masks")
    out = []
    for k, o in enumerate(ids.tolist()):
        if n[k] <= 0:
            continue
        x0, y0, x1, y1 = (int(v) for v in boxes[k])
        out.append({"scene_id": int(scene_id), "image_id": int(im_id), "category_id": int(o), "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1],
                    "score": float(score), "time": float(time), "segmentation": rle_from_mask(masks[k])})
    return out
