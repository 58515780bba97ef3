"""Render-and-compare verification of pose hypotheses: how well each posed model explains the image — its depth render held against
the detection's mask and, when there is one, the test depth image.  One raster call and one reduction per group of views.

The contract is "POSE VERIFICATION" of include/picopose_hip.h (csrc/pp_verify.hip; tests/verify_oracle.py restates it in numpy).  The
masks are bit-packed once per call by pp_rle_pack_bits from the run tables of masks.py (RunTable.pack); poses, cameras, windows, groups
and the depth conversion are scene.py's, as for evaluation.render_depth.

THIS IS THE PROJECT'S OWN RULE, not a published protocol's and not the reference's (which ranks hypotheses by the PnP inlier ratio
alone).  Detection masks are modal: they hold the visible part of an object only.  Without a depth image the render cannot be
clipped to what is visible, so the RGB-only `iou` penalises an occluded object — equally for all of its hypotheses, which leaves
their ranking meaningful but makes the value not comparable across instances.  Accuracy on real data is unmeasured and not claimed."""
import math

import numpy as np
import torch

from . import _lib
from . import scene as scn
from .masks import MAX_MASKS, RunTable, area_of_ends, rle_counts, run_ends
from .scene import DEFAULT_WORKSPACE_BYTES

COUNTS = ("render", "inter", "valid", "agree", "front", "behind", "vis", "vis_inter")       # the columns of `counts`


def _ratio(num, den, empty):
    """num / den in float64 where den > 0, `empty` elsewhere (torch tensors or numpy arrays of integers)."""
    if isinstance(num, torch.Tensor):
        n, d = num.to(torch.float64), den.to(torch.float64)
        return torch.where(d > 0, n / torch.where(d > 0, d, torch.ones_like(d)), torch.full_like(d, empty))
    n, d = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.where(d > 0, n / np.where(d > 0, d, 1.0), empty)


def scores(counts, area, with_depth):
    """counts (P, 8) integers (COUNTS), area (P,) the pixel count of each pose's mask -> (iou, visible_iou, agreement, score), each
    (P,) float64, from the integers alone:
      iou = inter / (render + A - inter), visible_iou = vis_inter / (vis + A - vis_inter)      (0 when the denominator is 0)
      agreement = agree / (agree + behind)                          (1 when agree + behind = 0: there is no depth evidence)
      score = visible_iou * agreement with a depth image, iou without.
    Torch tensors (any device) or numpy arrays; the same IEEE operations either way."""
    wide = (lambda a: a.to(torch.int64)) if isinstance(counts, torch.Tensor) else (lambda a: np.asarray(a, dtype=np.int64))
    c, area = [wide(counts[:, k]) for k in range(len(COUNTS))], wide(area)
    iou = _ratio(c[1], c[0] + area - c[1], 0.0)
    visible_iou = _ratio(c[7], c[6] + area - c[7], 0.0)
    agreement = _ratio(c[3], c[3] + c[5], 1.0)
    return iou, visible_iou, agreement, (visible_iou * agreement if with_depth else iou)


def _mask_index(mask_index, P, M):
    if mask_index is None:
        if M != P:
            raise ValueError(f"without mask_index every pose needs its own mask: {M} segmentations for {P} poses")
        return np.arange(P, dtype=np.int32)
    if isinstance(mask_index, torch.Tensor):
        mask_index = mask_index.cpu().numpy()
    idx = np.asarray(mask_index)
    if idx.shape != (P,) or (P and not np.issubdtype(idx.dtype, np.integer)):
        raise ValueError(f"mask_index must be {P} integers, got {idx.dtype} {idx.shape}")
    if P and (idx.min() < 0 or idx.max() >= M):
        raise ValueError(f"mask_index must lie in [0, {M})")
    return idx.astype(np.int32)


def _mask_runs(segmentations, H, W):
    """The cumulative run ends of every mask, each checked against the frame; ValueError names the mask."""
    runs = [run_ends(rle_counts(seg, i, "mask", (H, W))) for i, seg in enumerate(segmentations)]
    if len(runs) > MAX_MASKS:
        raise ValueError(f"at most {MAX_MASKS} masks per call, got {len(runs)}")
    return runs


def verify_poses(models, obj_ids, R, t, K, segmentations, size, mask_index=None, depth=None, image_index=None, depth_scale=None,
                 delta=15.0, near=1.0, window="auto", workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """P (object, pose) hypotheses against M detection masks of one (H, W) = size frame (and n_images depth images) ->
      {"counts": (P, 8) int32, the columns COUNTS = render, inter, valid, agree, front, behind, vis, vis_inter (include/picopose_hip.h,
       POSE VERIFICATION), "mask_area": (M,) int32, "iou", "visible_iou", "agreement", "score": (P,) float64 (see `scores`) — device
       tensors; "near_count": the triangles dropped at the near plane, "n_groups": the pp_pose_verify calls made}.

    segmentations: M COCO-RLE masks in any form masks.rle_counts accepts, each of `size`; mask_index (P,): the mask of
    each pose, so that the hypotheses of one detection share one mask (default: pose p has mask p, which needs M = P).
    R (P, 3, 3), t (P, 3) millimetres; K (3, 3) or (n_images, 3, 3) with image_index (P,) as evaluation.render_depth.
    depth: None (RGB only: score = iou) or (n_images, H, W) uint16 raw with `depth_scale` or float millimetres, as
    evaluation.vsd_errors takes it; a value that is not > 0 is missing.  delta (mm): a rendered sample more than delta behind the
    test depth is occluded (`front`), one more than delta in front of it is seen through (`behind`).  near and window as
    render_depth.  The views are processed in as many calls as `workspace_bytes` needs, with identical results.
    A pose whose window is empty (off the frame, a NaN or an infinity) has all-zero counts and score 0.  P = 0: empty tensors, no launch.
    ValueError before any device work: as render_depth, and for mismatched lengths, a mask whose size is not (H, W), more than
    4096 masks, a mask_index out of range, a depth image of another size, or a delta that is negative or not finite.

    This is the project's own rule (module docstring): detection masks are modal, so the RGB-only iou penalises an occluded object
    equally for all of its hypotheses — their ranking stays meaningful, the value is not comparable across instances — and accuracy on
    real data is unmeasured and not claimed."""
    obj = scn.obj_index(models, obj_ids)
    P, dev = len(obj), models.device
    scn.check_scalars(near, window, workspace_bytes)
    if not (isinstance(delta, (int, float)) and not isinstance(delta, bool) and math.isfinite(delta) and delta >= 0):
        raise ValueError(f"delta must be a non-negative number, got {delta!r}")
    res = scn.resolution_hw(size)
    if res is None or not scn.frame_in_range(*res):
        raise ValueError(f"size must be (H, W), positive with H W < 2^31, got {size!r}")
    H, W = res
    runs = _mask_runs(segmentations, H, W)
    M = len(runs)
    midx = _mask_index(mask_index, P, M)
    if depth is None:
        if depth_scale is not None:
            raise ValueError("depth_scale without depth")
        n_images, scale = scn.n_images_of(K), None
    else:
        n_images, Hd, Wd, scale = scn.check_depth(depth, depth_scale)
        if (Hd, Wd) != (H, W):
            raise ValueError(f"the depth images are {(Hd, Wd)}, the masks' frame is {(H, W)}")
    Rh, th = scn.host_f32("R", R, P, (3, 3)), scn.host_f32("t", t, P, (3,))
    cams = scn.cameras(K, n_images)
    img = scn.image_index(image_index, P, n_images)

    counts = torch.zeros((P, len(COUNTS)), dtype=torch.int32, device=dev)
    if P == 0:                                                    # (the areas from the runs: no launch)
        area = torch.tensor([area_of_ends(r) for r in runs], dtype=torch.int32, device=dev)
        iou, viou, agree, score = scores(counts, area[:0], depth is not None)
        return {"counts": counts, "mask_area": area, "iou": iou, "visible_iou": viou, "agreement": agree, "score": score,
                "near_count": 0, "n_groups": 0}
    poses = scn.pose44(Rh, th)
    windows = scn.view_windows(models, obj, img, poses, cams, H, W, near, window)
    groups = scn.view_groups(models, obj, windows, None, None, workspace_bytes)
    scn.require_gpu(dev)
    bits, area = RunTable.upload(runs, dev).pack(H * W)
    words = bits.shape[1]
    depth_d = None if depth is None else scn.depth_mm(depth, scale, dev)
    near_d = torch.empty((P,), dtype=torch.int32, device=dev)
    midx_d = torch.from_numpy(midx).to(dev)
    for views, _ in groups:
        v0, v1 = int(views[0]), int(views[-1]) + 1                # (consecutive views)
        packed = scn.PackedScene(models, cams, H, W, near, obj[v0:v1], img[v0:v1], poses[v0:v1], windows[v0:v1])
        ws = torch.empty(_lib.workspace_bytes("pp_vsd_workspace_bytes", packed.samples, packed.faces), dtype=torch.uint8, device=dev)
        vm = np.ascontiguousarray(midx[v0:v1])
        _lib.call("pp_pose_verify", packed.scene, bits, M, words, midx_d[v0:], vm, depth_d, float(delta), ws, ws.numel(), counts[v0:],
                  near_d[v0:])
    # the scores on the host, from the integers (the call reads near_count back anyway), then back beside the counts
    iou, viou, agree, score = (torch.from_numpy(a).to(dev) for a in scores(counts.cpu().numpy(), area.cpu().numpy()[midx], depth is not None))
    return {"counts": counts, "mask_area": area, "iou": iou, "visible_iou": viou, "agreement": agree, "score": score,
            "near_count": int(near_d.sum().item()), "n_groups": len(groups)}
