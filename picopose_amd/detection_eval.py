"""Score 2D detections and masks against ground truth: COCO-style average precision and recall, what BOP's detection and
segmentation tasks are scored by — for `depth_proposals.depth_proposals` (class_agnostic=True), `proposals.label_proposals`, or
any outside segmenter that writes CNOS / BOP detection records.

The contract is "DETECTION SCORING" of include/picopose_hip.h (csrc/pp_det_eval.hip; tests/detection_eval_oracle.py restates it in
numpy loops).  It is COCOeval WRITTEN FROM MEMORY: pycocotools and the BOP toolkit's eval_bop22_coco.py cannot be run next to this
library, so parity with both is UNPINNED.  What is exact: the overlaps and the match tables equal the restatement bit for bit.

The device computes the overlaps inside each (image, category) group (pp_rle_pack_bits, pp_det_overlaps) and the greedy matching per
(group, area range, threshold) (pp_det_match); grouping, sorting and chunking before, and the accumulation after, are numpy on the host."""
import json
import math
import os
import time

import numpy as np
import torch

from . import _lib
from . import scoring
from .masks import MAX_MASKS, RunTable, check_frame, rle_counts, rle_from_mask, run_ends
from . import scene_gt as sg

IOU_TYPES = ("segm", "bbox")
IOU_THRS = np.linspace(.5, .95, 10)
AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # COCO's all, small, medium, large
MAX_DETS = (1, 10, 100)
REC_THRS = scoring.REC_THRS
NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
DEFAULT_WORKSPACE_BYTES = 256 << 20
TILE = _lib.PP_DET_TILE
MAX_GT = _lib.PP_DET_MAX_GT
GT_IGNORE, GT_CROWD = 1, 2
_KEYS = ("scene_id", "image_id", "category_id", "bbox")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _check_record(rec, i, what, score):
    """The keys every record carries; ValueError names the record."""
    if not isinstance(rec, dict):
        raise ValueError(f"{what} {i}: a record is a dict, got {type(rec).__name__}")
    for k in _KEYS + (("score",) if score else ()):
        if k not in rec:
            raise ValueError(f"{what} {i}: no '{k}'")
    for k in _KEYS[:3]:
        if not _is_int(rec[k]):
            raise ValueError(f"{what} {i}: '{k}' must be an int, got {rec[k]!r}")
    try:
        box = [float(v) for v in rec["bbox"]]
    except (TypeError, ValueError):
        box = []
    if len(box) != 4 or not all(math.isfinite(v) for v in box) or box[2] < 0 or box[3] < 0:
        raise ValueError(f"{what} {i}: 'bbox' must be [x, y, w, h], finite with w, h >= 0, got {rec['bbox']!r}")
    if score:
        s = rec["score"]
        if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, float, np.integer, np.floating)) or not math.isfinite(s):
            raise ValueError(f"{what} {i}: 'score' must be a finite number, got {s!r}")
    return box


def read_detections(path_or_records):
    """CNOS / BOP detection JSON (a path, or the decoded list) -> the list of records, each checked for scene_id, image_id,
    category_id (ints), bbox [x, y, w, h], score and segmentation ({"size": [h, w], "counts": ...}); ValueError names the record."""
    recs = path_or_records
    if isinstance(recs, (str, bytes, os.PathLike)):
        with open(recs) as f:
            recs = json.load(f)
    if not isinstance(recs, (list, tuple)):
        raise ValueError(f"detections must be a list of records, got {type(recs).__name__}")
    for i, r in enumerate(recs):
        _check_record(r, i, "detection", True)
        seg = r.get("segmentation")
        if not isinstance(seg, dict) or "size" not in seg or "counts" not in seg:
            raise ValueError(f"detection {i}: 'segmentation' must be {{'size': [h, w], 'counts': ...}}")
    return list(recs)


def _annotations(ids, masks, boxes, counts, fract, scene_id, im_id, min_visib_fract):
    out = []
    for k, o in enumerate(ids):
        if counts[k] <= 0:
            continue
        x0, y0, x1, y1 = (int(v) for v in boxes[k])
        out.append({"scene_id": int(scene_id), "image_id": int(im_id), "category_id": int(o), "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1],
                    "segmentation": rle_from_mask(masks[k]), "ignore": bool(fract[k] < min_visib_fract), "iscrowd": False})
    return out


def gt_annotations(obj_ids, result, scene_id, im_id, min_visib_fract=0.1):
    """Ground-truth annotations of one image: obj_ids (U,) and result = scene_gt.scene_gt_info(..., masks="visib" or "both") of that
    image's instances -> a list of {"scene_id", "image_id", "category_id", "bbox" [x, y, w, h] of the visible mask, "segmentation"
    (the visible mask), "ignore", "iscrowd": False} in instance order — `scene_gt.gt_detections`' records without score and time.  An
    instance with an empty visible mask is left out; ignore = visib_fract < min_visib_fract: BOP's rule AS REMEMBERED (an instance
    seen less than 10 % is neither required nor penalised; parity unpinned)."""
    if "mask_visib" not in result:
        raise ValueError("gt_annotations needs scene_gt_info(..., masks='visib' or 'both')")
    ids = np.asarray(obj_ids.cpu() if isinstance(obj_ids, torch.Tensor) else obj_ids).reshape(-1)
    masks = sg._np(result["mask_visib"])
    if len(ids) != len(masks):
        raise ValueError(f"{len(ids)} obj_ids for {len(masks)} masks")
    return _annotations(ids.tolist(), masks, sg._np(result["bbox_visib"]), sg._np(result["px_count_visib"]),
                        np.asarray(result["visib_fract"], np.float64), scene_id, im_id, min_visib_fract)


def dataset_annotations(ground_truth, cameras, models, resolution, depth_images=None, images_per_call=64, min_visib_fract=0.1, **kw):
    """Ground-truth annotations of whole scenes, a flat list in (scene, image, instance) order: `scene_gt.dataset_gt_info`'s
    arguments and batching (one scene_gt_info call per `images_per_call` images, masks="visib"; kw goes to it), then
    `gt_annotations`' rule per image."""
    if "masks" in kw:
        raise ValueError("dataset_annotations chooses masks='visib' itself")
    out = []
    for batch, obj, r in sg.dataset_gt_batches(ground_truth, cameras, models, resolution, depth_images, images_per_call, masks="visib", **kw):
        masks, boxes, counts = sg._np(r["mask_visib"]), sg._np(r["bbox_visib"]), sg._np(r["px_count_visib"])
        k = 0
        for (s, im), o in zip(batch, obj):
            e = k + len(o)
            out += _annotations(o.tolist(), masks[k:e], boxes[k:e], counts[k:e], r["visib_fract"][k:e], s, im, min_visib_fract)
            k = e
    return out


def _settings(iou_type, iou_thrs, area_ranges, max_dets, workspace_bytes):
    if iou_type not in IOU_TYPES:
        raise ValueError(f"iou_type must be one of {IOU_TYPES}, got {iou_type!r}")
    thrs = np.ascontiguousarray(IOU_THRS if iou_thrs is None else iou_thrs, dtype=np.float64).reshape(-1)
    if thrs.size == 0 or not np.all((thrs > 0) & (thrs <= 1)):
        raise ValueError(f"iou_thrs must be a non-empty list of values in (0, 1], got {iou_thrs!r}")
    ranges = np.ascontiguousarray(AREA_RANGES if area_ranges is None else area_ranges, dtype=np.float64)
    if ranges.ndim != 2 or ranges.shape[1] != 2 or ranges.shape[0] == 0 or not np.all(ranges[:, 0] <= ranges[:, 1]):
        raise ValueError(f"area_ranges must be a non-empty list of [lo, hi] with lo <= hi, got {area_ranges!r}")
    try:
        md = tuple(max_dets)
    except TypeError:
        md = ()
    if not md or not all(_is_int(m) and m > 0 for m in md):
        raise ValueError(f"max_dets must be a non-empty list of positive ints, got {max_dets!r}")
    if not (_is_int(workspace_bytes) and workspace_bytes > 0):
        raise ValueError(f"workspace_bytes must be a positive int, got {workspace_bytes!r}")
    return thrs, ranges, tuple(int(m) for m in md)


class _Side:
    """The parsed records of one side: image key, category, box, run ends, mask area and frame size per record."""

    def __init__(self, records, what, segm, need_area, class_agnostic, sizes):
        n = len(records)
        self.key, self.cat, self.box = [None] * n, np.zeros(n, np.int64), np.zeros((n, 4), np.float64)
        self.runs, self.area, self.score = [None] * n, np.zeros(n, np.float64), np.zeros(n, np.float64)
        self.flags = np.zeros(n, np.uint8)
        for i, r in enumerate(records):
            self.box[i] = _check_record(r, i, what, what == "detection")
            self.key[i] = (int(r["scene_id"]), int(r["image_id"]))
            self.cat[i] = 0 if class_agnostic else int(r["category_id"])
            if what == "detection":
                self.score[i] = float(r["score"])
            else:
                crowd = bool(r.get("iscrowd", False))
                self.flags[i] = (GT_IGNORE if (bool(r.get("ignore", False)) or crowd) else 0) | (GT_CROWD if crowd else 0)
            if segm or need_area:
                if "segmentation" not in r:
                    raise ValueError(f"{what} {i}: no 'segmentation'")
                counts = rle_counts(r["segmentation"], i, what, sizes.get(self.key[i]) if segm else None)
                h, w = (int(v) for v in r["segmentation"]["size"])
                if segm:
                    check_frame(h, w)
                    sizes.setdefault(self.key[i], (h, w))
                    self.runs[i] = run_ends(counts)
                self.area[i] = float(counts[1::2].sum())                      # the odd runs are the runs of ones
            if not (segm or need_area):
                self.area[i] = self.box[i, 2] * self.box[i, 3]


def _tiles(groups):
    """groups (n, 5) -> the (n_tiles, 3) list {group, first detection, first ground truth} of the TILE x TILE tiles that hold a pair."""
    ti, tj = (groups[:, 1] + TILE - 1) // TILE, (groups[:, 3] + TILE - 1) // TILE
    nt = ti * tj
    if nt.sum() == 0:
        return np.zeros((0, 3), np.int32)
    g = np.repeat(np.arange(len(groups)), nt)
    k = np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)
    return np.ascontiguousarray(np.stack([g, (k // tj[g]) * TILE, (k % tj[g]) * TILE], axis=1), dtype=np.int32)


def _run_chunk(dev, segm, hw, runs, boxes, groups, flags, det_area, gt_area, ranges, thrs, timings=None):
    """One chunk on the device: (pack,) overlaps, match -> (inter or None, iou, dt_match, dt_ignore, gt_match, gt_ignore) as numpy.
    timings: a dict that receives the device seconds of the pack, overlaps and match launches (event pairs on the current stream)."""
    mark, finish = scoring.device_marks(timings)
    n_groups = len(groups)
    n_det, n_gt = len(det_area), len(gt_area)
    n_pairs = int((groups[:, 1] * groups[:, 3]).sum())
    scoring.check_offsets(n_pairs, "chunk")
    A, T = len(ranges), len(thrs)
    up = scoring.uploader(dev)
    tiles = _tiles(groups)
    groups_d, flags_d = up(groups.ravel()), up(flags, side=True)
    tiles_d = up(tiles.ravel()) if len(tiles) else None
    iou = torch.zeros(max(n_pairs, 1), dtype=torch.float64, device=dev)
    inter = bits = area = boxes_d = None
    words = 0
    if segm:
        words = (hw + 31) // 32
        table = RunTable.upload(runs, dev)
        mark("pack")
        bits, area = table.pack(hw)
        mark("pack")
        inter = torch.zeros(max(n_pairs, 1), dtype=torch.int32, device=dev)
    else:
        boxes_d = up(boxes.ravel())
    mark("overlaps")
    _lib.call("pp_det_overlaps", bits, area, words, boxes_d, n_det, n_gt, groups_d, groups, n_groups, tiles_d, tiles, len(tiles), flags_d,
              n_pairs, inter, iou)
    mark("overlaps")
    da_d, ga_d = up(det_area, side=True), up(gt_area, side=True)
    ranges_d, thrs_d = up(ranges.ravel()), up(thrs)
    dt_match = torch.full((A, T, max(n_det, 1)), -1, dtype=torch.int32, device=dev)
    dt_ignore = torch.zeros((A, T, max(n_det, 1)), dtype=torch.uint8, device=dev)
    gt_match = torch.full((A, T, max(n_gt, 1)), -1, dtype=torch.int32, device=dev)
    gt_ignore = torch.zeros((A, max(n_gt, 1)), dtype=torch.uint8, device=dev)
    mark("match")
    _lib.call("pp_det_match", iou, n_pairs, groups_d, groups, n_groups, n_det, n_gt, da_d, ga_d, flags_d, ranges_d, ranges, A, thrs_d, thrs, T,
              dt_match, dt_ignore, gt_match, gt_ignore)
    mark("match")
    finish()
    host = lambda t, n: t.cpu().numpy()[..., :n]      # noqa: E731
    return (host(inter, n_pairs) if segm else None, host(iou, n_pairs), host(dt_match, n_det), host(dt_ignore, n_det), host(gt_match, n_gt),
            host(gt_ignore, n_gt))


def match_detections(detections, annotations, iou_type="segm", iou_thrs=None, area_ranges=None, max_dets=MAX_DETS, class_agnostic=False,
                     device="cuda", workspace_bytes=DEFAULT_WORKSPACE_BYTES, timings=None):
    """Detections (CNOS records) against ground-truth annotations (`gt_annotations`' records) -> the match tables of DETECTION
    SCORING and everything `accumulate` needs, numpy arrays on the host:
      "images": the sorted (scene_id, image_id) keys, "categories": the sorted category ids, "iou_type", "iou_thrs" (T,), "area_ranges"
      (A, 2), "max_dets"; one GROUP per (image, category) that holds a record, sorted by (image, category): "group_image", "group_category"
      (indices into the two lists), "group_det" and "group_gt" (n_groups, 2) = {first, count} on the detection / ground-truth axis,
      "group_pair" the offset of the group's D_g x G_g row-major block in "inter" (int32; None for bbox) and "iou" (float64);
      the DETECTION axis holds each group's detections by descending score (the lower input index first among equal scores), cut to
      max(max_dets): "det_index" (the input index) and "det_score"; the GROUND-TRUTH axis holds each group's annotations in input order:
      "gt_index"; "dt_match" (A, T, n_det) int32 = the position on the ground-truth axis of the matched annotation or -1, "dt_ignore"
      (A, T, n_det) uint8, "gt_match" (A, T, n_gt) int32 = the position on the detection axis or -1, "gt_ignore" (A, n_gt) uint8.
    class_agnostic=True puts every record in category 0 (what scores `depth_proposals` before labelling).  A crowd annotation is ignored
    as well.  segm: the masks are bit-packed per chunk of whole images that share a frame size (at most 4096 masks and about
    `workspace_bytes` of device tables per chunk; one image always runs, whatever the bound); a mask whose size differs from its
    image's other masks raises `masks.rle_counts`' error.  timings: a dict that receives the device seconds of the pack, overlaps and
    match launches, summed over the chunks, and "total", the wall-clock seconds of the whole call.  bbox: annotations still need their segmentation (their area is the mask's
    pixel count), detections do not.  The tables do not depend on the chunking.  ValueError names the offending record."""
    t_start = time.perf_counter()
    thrs, ranges, max_dets = _settings(iou_type, iou_thrs, area_ranges, max_dets, workspace_bytes)
    if not isinstance(detections, (list, tuple)) or not isinstance(annotations, (list, tuple)):
        raise ValueError("detections and annotations must be lists of records")
    segm = iou_type == "segm"
    sizes = {}
    D = _Side(detections, "detection", segm, False, class_agnostic, sizes)
    G = _Side(annotations, "annotation", segm, True, class_agnostic, sizes)
    images = sorted(set(D.key) | set(G.key))
    cats = sorted(set(D.cat.tolist()) | set(G.cat.tolist()))
    img_of, cat_of = {k: i for i, k in enumerate(images)}, {c: i for i, c in enumerate(cats)}
    members = {}
    for side, S in enumerate((D, G)):
        for n in range(len(S.key)):
            members.setdefault((img_of[S.key[n]], cat_of[int(S.cat[n])]), ([], []))[side].append(n)
    cut = max(max_dets)
    A, T = len(ranges), len(thrs)
    keys = sorted(members)
    g_img, g_cat = np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64)
    sides = [[np.array(m, np.int64) for m in members[k]] for k in keys]
    det_lists, gt_lists = [d[np.argsort(-D.score[d], kind="stable")][:cut] for d, _ in sides], [g for _, g in sides]
    group_det, group_gt, p0, det_index, gt_index, n_pairs = scoring.plan_groups([(images[i], cats[c]) for i, c in keys], det_lists, gt_lists,
                                                                                MAX_GT, "category", "annotations")
    (d0, nd), (g0, ng), n_det, n_gt = group_det.T, group_gt.T, len(det_index), len(gt_index)
    out = {"iou_type": iou_type, "iou_thrs": thrs, "area_ranges": ranges, "max_dets": max_dets, "images": images, "categories": cats,
           "group_image": g_img, "group_category": g_cat, "group_det": group_det, "group_gt": group_gt, "group_pair": p0,
           "det_index": det_index, "gt_index": gt_index, "det_score": D.score[det_index],
           "inter": np.zeros(n_pairs, np.int32) if segm else None, "iou": np.zeros(n_pairs, np.float64),
           "dt_match": np.full((A, T, n_det), -1, np.int32), "dt_ignore": np.zeros((A, T, n_det), np.uint8),
           "gt_match": np.full((A, T, n_gt), -1, np.int32), "gt_ignore": np.zeros((A, n_gt), np.uint8), "n_chunks": 0}
    if not keys:
        return out
    # chunks: runs of whole images of one frame size (bbox: any), in image order
    det_area = D.area[det_index] if n_det else np.zeros(0)
    per_image = {}
    for q, k in enumerate(keys):
        per_image.setdefault(k[0], []).append(q)
    chunks, cur = [], {}
    for i in sorted(per_image):
        qs = per_image[i]
        size = sizes.get(images[i]) if segm else None
        words = (size[0] * size[1] + 31) // 32 if segm else 0
        masks = int(nd[qs].sum() + ng[qs].sum())
        if segm and masks > MAX_MASKS:
            raise ValueError(f"image {images[i]}: {masks} masks after the max_dets cut, more than the {MAX_MASKS} of one pack call")
        cost = masks * (4 * words + 48) + int((nd[qs] * ng[qs]).sum()) * 12 + A * T * int(5 * nd[qs].sum() + 4 * ng[qs].sum())
        c = cur.get(size)
        if c is not None and (c[1] + cost > workspace_bytes or (segm and c[2] + masks > MAX_MASKS)):
            chunks.append((size, c[0]))
            c = None
        if c is None:
            c = cur[size] = [[], 0, 0]
        c[0] += qs
        c[1] += cost
        c[2] += masks
    chunks += [(size, c[0]) for size, c in cur.items()]
    dev = scoring.require_cuda(device, "match_detections")
    for size, qs in chunks:
        qs = np.array(qs, np.int64)
        cd, cg = nd[qs], ng[qs]
        groups = scoring.group_rows(*(np.stack([scoring.first(c), c], axis=1) for c in (cd, cg)), scoring.first(cd * cg))
        span = lambda s, c: np.concatenate([np.arange(a, a + b) for a, b in zip(s, c)]) if c.sum() else np.zeros(0, np.int64)  # noqa: E731
        dpos, gpos, ppos = span(d0[qs], cd), span(g0[qs], cg), span(p0[qs], cd * cg)
        di, gi = det_index[dpos], gt_index[gpos]
        runs = [D.runs[n] for n in di] + [G.runs[n] for n in gi] if segm else None
        boxes = None if segm else np.concatenate([D.box[di], G.box[gi]])
        inter, iou, dtm, dtig, gtm, gtig = _run_chunk(dev, segm, size[0] * size[1] if segm else 0, runs, boxes, groups,
                                                      G.flags[gi], det_area[dpos], G.area[gi], ranges, thrs, timings)
        if segm:
            out["inter"][ppos] = inter
        out["iou"][ppos] = iou
        out["dt_match"][:, :, dpos] = np.where(dtm >= 0, gpos[np.maximum(dtm, 0)] if len(gpos) else -1, -1)
        out["dt_ignore"][:, :, dpos] = dtig
        out["gt_match"][:, :, gpos] = np.where(gtm >= 0, dpos[np.maximum(gtm, 0)] if len(dpos) else -1, -1)
        out["gt_ignore"][:, gpos] = gtig
        out["n_chunks"] += 1
    if timings is not None:
        timings["total"] = timings.get("total", 0.0) + time.perf_counter() - t_start
    return out


def accumulate(matches):
    """match_detections' result -> {"precision" (T, 101, K, A, M), "recall" (T, K, A, M)} float64 (and the settings `summarize` reads),
    K the categories, M the max_dets values: per category, area range and max_dets value the first max_det detections of every
    image, sorted by descending score (mergesort); a cell without a non-ignored ground truth stays -1."""
    m = matches
    thrs, ranges, max_dets, cats = m["iou_thrs"], m["area_ranges"], m["max_dets"], m["categories"]
    T, A, M, K = len(thrs), len(ranges), len(max_dets), len(cats)
    precision, recall = -np.ones((T, 101, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        rows = np.nonzero(m["group_category"] == k)[0]
        gsel = np.concatenate([np.arange(s, s + n) for s, n in m["group_gt"][rows]] + [np.zeros(0, np.int64)]).astype(np.int64)
        for a in range(A):
            npig = int(np.count_nonzero(m["gt_ignore"][a, gsel] == 0))
            if npig == 0:
                continue
            for mi, md in enumerate(max_dets):
                sel = np.concatenate([np.arange(s, s + min(n, md)) for s, n in m["group_det"][rows]] + [np.zeros(0, np.int64)]).astype(np.int64)
                sel = sel[np.argsort(-m["det_score"][sel], kind="mergesort")]
                precision[:, :, k, a, mi], recall[:, k, a, mi] = scoring.pr_curve(m["dt_match"][a][:, sel] >= 0, m["dt_ignore"][a][:, sel] != 0, npig)
    return {"precision": precision, "recall": recall, "iou_thrs": thrs, "area_ranges": ranges, "max_dets": max_dets, "categories": cats}


def summarize(acc):
    """accumulate's result -> the twelve COCO numbers {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm",
    "ARl"} and "per_object_AP" {category id: AP}.  Each is the mean of the cells > -1, or -1 when there is none.  The area ranges and
    max_dets are read BY POSITION — all, small, medium, large and 1, 10, 100, COCO's defaults: AP* take the last max_dets value, AP50 /
    AP75 the thresholds equal to 0.5 / 0.75, ARs / ARm / ARl the last max_dets value; a position that the settings lack gives -1."""
    p, r, thrs = acc["precision"], acc["recall"], acc["iou_thrs"]
    A, M = p.shape[3], p.shape[4]

    def ap(a, thr=None):
        if a >= A:
            return -1.0
        t = slice(None) if thr is None else np.where(thrs == thr)[0]
        return scoring.mean_valid(p[t, :, :, a, M - 1])

    def ar(a, mi):
        return scoring.mean_valid(r[:, :, a, mi]) if a < A and mi < M else -1.0

    out = dict(zip(NAMES, [ap(0), ap(0, .5), ap(0, .75), ap(1), ap(2), ap(3), ar(0, 0), ar(0, 1), ar(0, 2), ar(1, M - 1), ar(2, M - 1), ar(3, M - 1)]))
    out["per_object_AP"] = {c: scoring.mean_valid(p[:, :, k, 0, M - 1]) for k, c in enumerate(acc["categories"])}
    return out


def score_detections(detections, annotations, **kw):
    """summarize(accumulate(match_detections(detections, annotations, **kw))): the twelve numbers and per-object AP in one call."""
    return summarize(accumulate(match_detections(detections, annotations, **kw)))
