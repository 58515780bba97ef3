"""Class-agnostic mask proposals from the depth image alone: the segmenter that `proposals.label_proposals` was missing.

Per image: the dominant plane (the table, the bin floor) by a consensus over hashed three-pixel hypotheses and a float64 refit; the
valid pixels that stand between `min_height` and `max_height` over it, within `max_range`, are foreground; foreground 4-neighbours
whose depths differ by at most `max_step` are connected; every component of a plausible size becomes one COCO-RLE proposal.

THIS IS THE PROJECT'S OWN ALGORITHM — a classical depth clusterer, as `verify`, `rgbd_pose` and `depth_refine` are the project's own
rules — and claims parity with no published segmenter.  What is exact: the contract is "DEPTH PROPOSALS" of include/picopose_hip.h
(csrc/pp_depth_proposals.hip), and tests/depth_proposals_oracle.py restates it in numpy; scores, labels, records and run lengths equal
that restatement bit for bit, the plane is a float64 fit.  What is NOT claimed: accuracy on real depth images is unmeasured; objects
that touch at equal depth come out as one proposal, and the defaults below are settings in millimetres, not measured optima.

`plane_fit`, `components`, `component_stats` and `component_rle` wrap one ABI entry each; `depth_proposals` composes them with two
host reads (the compact records, then the run counts)."""
import math

import numpy as np
import torch

from . import _lib
from . import scene as scn
from .masks import MAX_MASKS, RunTable, counts_of_ends

MAX_HYP = _lib.PP_PLANE_MAX_HYP
FIELDS = ("root", "area", "xmin", "ymin", "xmax", "ymax", "border")        # the columns of component_stats' records


def _number(name, v, lo=None, strict=False):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    if lo is not None and (v <= lo if strict else v < lo):
        raise ValueError(f"{name} must be {'>' if strict else '>='} {lo}, got {v!r}")
    return float(v)


def _integer(name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{name} must be an integer in [{lo}, {'...' if hi is None else hi}], got {v!r}")
    return int(v)


def _frames(name, t, dtype):
    """(B, H, W) of a tensor that must be a contiguous (B, H, W) `dtype` tensor; the device is checked last, by the caller."""
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype != dtype or 0 in t.shape:
        raise ValueError(f"{name} must be a non-empty (B, H, W) {dtype} tensor")
    B, H, W = (int(v) for v in t.shape)
    if H * W >= 2 ** 31 or B > 65535:
        raise ValueError(f"{name}: at most 65535 frames of fewer than 2^31 pixels")
    return B, H, W


def _cams(cams, B):
    if not isinstance(cams, torch.Tensor) or cams.dtype != torch.float32 or tuple(cams.shape) != (B, 4):
        raise ValueError(f"cams must be a ({B}, 4) float32 tensor of fx, fy, cx, cy")
    return cams


def _device_tensors(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise _lib.PicoPoseHipError("picopose_amd runs on the GPU only: inputs must be CUDA(HIP) tensors")
    return [t.contiguous() for t in tensors]


def plane_fit(depth, cams, *, tau=5.0, n_hyp=256, seed=0, min_inliers=1000):
    """depth (B, H, W) float32 millimetres and cams (B, 4) float32 {fx, fy, cx, cy}, both on the device -> {"plane": (B, 4) float32
    (n, d) with n . p + d = 0 and the camera on the positive side, "plane64": the float64 fit it is the cast of, "info": (B, 4) int32 =
    has_plane, winner, the winner's inlier count, the refit's consensus count} (pp_depth_plane; nothing waits for the device).
    An image whose best hypothesis has fewer than `min_inliers` inliers has no plane: a zero row and has_plane 0.
    ValueError before any device work: shapes and dtypes, tau negative or not finite, n_hyp outside [1, 1024], min_inliers < 3, a seed
    outside 32 bits."""
    B, H, W = _frames("depth", depth, torch.float32)
    _cams(cams, B)
    tau = _number("tau", tau, 0.0)
    n_hyp, seed, min_inliers = _integer("n_hyp", n_hyp, 1, MAX_HYP), _integer("seed", seed, 0, 2 ** 32 - 1), _integer("min_inliers", min_inliers, 3, 2 ** 31 - 1)
    depth, cams = _device_tensors(depth, cams)
    dev = depth.device
    ws = torch.empty(_lib.workspace_bytes("pp_depth_plane_workspace_bytes", B, H, W, n_hyp), dtype=torch.uint8, device=dev)
    plane = torch.empty((B, 4), dtype=torch.float32, device=dev)
    plane64 = torch.empty((B, 4), dtype=torch.float64, device=dev)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    _lib.call("pp_depth_plane", depth, cams, B, H, W, n_hyp, seed, tau, min_inliers, ws, ws.numel(), plane, plane64, info)
    return {"plane": plane, "plane64": plane64, "info": info}


def components(depth, cams, plane, has_plane, *, min_height=10.0, max_height=400.0, max_range=3000.0, max_step=15.0):
    """depth, cams as plane_fit; plane (B, 4) float32 and has_plane (B,) int32 on the device -> labels (B, H, W) int32: -1 for
    background, otherwise the smallest row-major pixel index of the pixel's 4-connected foreground component (pp_depth_components).
    ValueError before any device work: shapes and dtypes, a height bound that is not finite or min_height >= max_height, max_range not
    positive, max_step negative."""
    B, H, W = _frames("depth", depth, torch.float32)
    _cams(cams, B)
    if not isinstance(plane, torch.Tensor) or plane.dtype != torch.float32 or tuple(plane.shape) != (B, 4):
        raise ValueError(f"plane must be a ({B}, 4) float32 tensor")
    if not isinstance(has_plane, torch.Tensor) or has_plane.dtype != torch.int32 or tuple(has_plane.shape) != (B,):
        raise ValueError(f"has_plane must be a ({B},) int32 tensor")
    lo, hi = _number("min_height", min_height), _number("max_height", max_height)
    if lo >= hi:
        raise ValueError(f"min_height {lo} must be below max_height {hi}")
    max_range, max_step = _number("max_range", max_range, 0.0, strict=True), _number("max_step", max_step, 0.0)
    if H > 32 * 65535:
        raise ValueError("frames of more than 32 * 65535 rows are not supported")
    depth, cams, plane, has_plane = _device_tensors(depth, cams, plane, has_plane)
    nbytes = _lib.workspace_bytes("pp_depth_components_workspace_bytes", B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=depth.device) if nbytes else None
    labels = torch.empty((B, H, W), dtype=torch.int32, device=depth.device)
    _lib.call("pp_depth_components", depth, cams, plane, has_plane, B, H, W, lo, hi, max_range, max_step, ws, nbytes, labels)
    return labels


def component_stats(labels, *, min_area=1, max_area=None, drop_border=False, cap=1024):
    """labels (B, H, W) int32 as `components` writes them -> (n_qualified (B,) int32, records (B, cap, 7) int32) on the device
    (pp_component_stats): per image the components with min_area <= area <= max_area (default: any), not touching the frame border when
    drop_border; a record is FIELDS = root, area, xmin, ymin, xmax, ymax (inclusive), border.  Only the first min(n_qualified, cap)
    records of an image are written, in no particular order; n_qualified counts all that qualified, so overflow is visible.
    ValueError before any device work: shape and dtype, min_area < 1, max_area < min_area, cap < 1."""
    B, H, W = _frames("labels", labels, torch.int32)
    min_area = _integer("min_area", min_area, 1, 2 ** 31 - 1)
    max_area = _integer("max_area", H * W if max_area is None else max_area, min_area, 2 ** 31 - 1)
    cap = _integer("cap", cap, 1, 2 ** 24)
    (labels,) = _device_tensors(labels)
    dev = labels.device
    ws = torch.empty(_lib.workspace_bytes("pp_component_stats_workspace_bytes", B, H, W), dtype=torch.uint8, device=dev)
    n_q = torch.empty((B,), dtype=torch.int32, device=dev)
    recs = torch.empty((B, cap, len(FIELDS)), dtype=torch.int32, device=dev)
    _lib.call("pp_component_stats", labels, B, H, W, min_area, max_area, int(bool(drop_border)), cap, ws, ws.numel(), n_q, recs)
    return n_q, recs


def component_rle(labels, selection):
    """labels (B, H, W) int32 and selection (n, 6) integers on the host = image, root, xmin, ymin, xmax, ymax (the box must hold the
    component: component_stats' is) -> the masks.RunTable (ends, offset, offset_host, n_runs) of the components' cumulative COCO run
    ends, so they feed pp_rle_pack_bits and pp_detections_crop unchanged (pp_components_rle: a count pass, one host read of the
    counts, an emit pass).
    ValueError before any device work: shapes, n outside [1, 4096], an image, root or box outside the frame."""
    B, H, W = _frames("labels", labels, torch.int32)
    sel = np.asarray(selection)
    if sel.ndim != 2 or sel.shape[1] != 6 or not np.issubdtype(sel.dtype, np.integer) or not 1 <= len(sel) <= MAX_MASKS:
        raise ValueError(f"selection must be (n, 6) integers with 1 <= n <= {MAX_MASKS}")
    sel = np.ascontiguousarray(sel, dtype=np.int32)
    b, root, x0, y0, x1, y1 = sel.T.astype(np.int64)
    if ((b < 0) | (b >= B) | (root < 0) | (root >= H * W) | (x0 < 0) | (x0 > x1) | (x1 >= W) | (y0 < 0) | (y0 > y1) | (y1 >= H)).any():
        raise ValueError("selection: an image, root or box outside the frame")
    (labels,) = _device_tensors(labels)
    dev, n = labels.device, len(sel)
    sel_d = torch.from_numpy(sel).to(dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    _lib.call("pp_components_rle", labels, B, H, W, sel_d, sel, n, None, None, 0, counts, None)
    off = np.zeros(n + 1, np.int32)
    np.cumsum(counts.cpu().numpy(), out=off[1:])
    table = RunTable.from_words(torch.empty((int(off[-1]) + n + 1,), dtype=torch.int32, device=dev), off)
    table.offset.copy_(torch.from_numpy(off))
    _lib.call("pp_components_rle", labels, B, H, W, sel_d, sel, n, table.offset, off, table.n_runs, None, table.ends)
    return table


def sort_records(records, max_proposals):
    """(k, 7) records of one image on the host -> the `max_proposals` largest, by area descending and then by root ascending."""
    order = np.lexsort((records[:, 0], -records[:, 1].astype(np.int64)))
    return records[order[:max_proposals]]


def depth_proposals(depth, K, *, depth_scale=None, tau=5.0, n_hyp=256, seed=0, min_inliers=1000, min_height=10.0, max_height=400.0,
                    max_range=3000.0, max_step=15.0, min_area_px=200, max_area_frac=0.5, drop_border=False, max_proposals=200, device="cuda"):
    """One depth image (H, W), or a batch (B, H, W), and its camera(s) K (3, 3) or (B, 3, 3) -> mask proposals, largest first:
    a list of {"segmentation": {"size": [H, W], "counts": [...]} (uncompressed COCO RLE), "bbox": [x, y, w, h], "area": int}
    (a list of such lists for a batch).  `proposals.label_proposals` and `pipeline.infer_proposals` take the list as it is.
    depth: uint16 raw with `depth_scale`, or float millimetres, numpy or torch, as `verify.verify_poses` takes it.

    The settings, in millimetres; they are settings for table-top and bin scenes, NOT measured optima (module docstring):
      tau 5           a pixel within 5 mm of a hypothesis's plane is its inlier (sensor noise at about a metre)
      n_hyp 256, seed the hashed three-pixel hypotheses per image (at most 1024)
      min_inliers 1000  fewer inliers than this: the image has no plane and only max_range applies
      min_height 10, max_height 400   foreground stands more than 10 and less than 400 mm over the plane, on the camera's side
      max_range 3000  farther pixels are background
      max_step 15     4-neighbours whose depths differ by more than 15 mm are not connected (an occlusion edge)
      min_area_px 200, max_area_frac 0.5   components of fewer pixels, or of more than that fraction of the frame, are dropped
      drop_border     drop components that touch the frame border (truncated objects)
      max_proposals 200   the largest are kept (area descending, then the component's first pixel ascending)
    ValueError before any device work for a setting out of range.  Objects that touch at equal depth are ONE proposal; accuracy on
    real depth images is unmeasured and not claimed."""
    single = getattr(depth, "ndim", 0) == 2
    if single:
        depth = depth[None]
    B, H, W, scale = scn.check_depth(depth, depth_scale)
    cams = scn.cameras(K, B)
    frac = _number("max_area_frac", max_area_frac, 0.0, strict=True)
    if frac > 1.0:
        raise ValueError(f"max_area_frac must be at most 1, got {max_area_frac!r}")
    min_area = _integer("min_area_px", min_area_px, 1, 2 ** 31 - 1)
    max_area = int(frac * H * W)
    if max_area < min_area:
        raise ValueError(f"max_area_frac {frac} of {H} x {W} pixels is below min_area_px {min_area}")
    max_proposals = _integer("max_proposals", max_proposals, 1, MAX_MASKS)
    # the stages check their own settings; repeated here so that a bad one is reported before the depth image is uploaded
    _number("tau", tau, 0.0), _integer("n_hyp", n_hyp, 1, MAX_HYP), _integer("seed", seed, 0, 2 ** 32 - 1), _integer("min_inliers", min_inliers, 3)
    if _number("min_height", min_height) >= _number("max_height", max_height):
        raise ValueError(f"min_height {min_height} must be below max_height {max_height}")
    _number("max_range", max_range, 0.0, strict=True), _number("max_step", max_step, 0.0)
    dev = torch.device(device)
    scn.require_gpu(dev)

    depth_d = scn.depth_mm(depth, scale, dev)
    cams_d = torch.from_numpy(cams).to(dev)
    fit = plane_fit(depth_d, cams_d, tau=tau, n_hyp=n_hyp, seed=seed, min_inliers=min_inliers)
    labels = components(depth_d, cams_d, fit["plane"], fit["info"][:, 0].contiguous(), min_height=min_height, max_height=max_height,
                        max_range=max_range, max_step=max_step)
    cap = max(1, min(H * W // min_area, 4096))                                # (no more than H W / min_area components can qualify)
    n_q, recs = component_stats(labels, min_area=min_area, max_area=max_area, drop_border=drop_border, cap=cap)
    n_q = n_q.cpu().numpy()
    if int(n_q.max()) > cap:                                                   # which records an overflowing list keeps is unspecified: take all
        cap = int(n_q.max())
        recs = component_stats(labels, min_area=min_area, max_area=max_area, drop_border=drop_border, cap=cap)[1]
    recs = recs.cpu().numpy()
    kept = [sort_records(recs[b, :min(int(n_q[b]), cap)], max_proposals) for b in range(B)]
    out = [[] for _ in range(B)]
    flat = [(b, r) for b in range(B) for r in kept[b]]
    for s in range(0, len(flat), MAX_MASKS):                                   # one count and one emit launch per MAX_MASKS components
        part = flat[s:s + MAX_MASKS]
        sel = np.array([[b, r[0], r[2], r[3], r[4], r[5]] for b, r in part], dtype=np.int32)
        table = component_rle(labels, sel)
        ends, off = table.ends.cpu().numpy(), table.offset_host
        for k, (b, r) in enumerate(part):
            out[b].append({"segmentation": {"size": [H, W], "counts": counts_of_ends(ends[off[k]:off[k + 1]]).tolist()},
                           "bbox": [int(r[2]), int(r[3]), int(r[4] - r[2] + 1), int(r[5] - r[3] + 1)], "area": int(r[1])})
    return out[0] if single else out
