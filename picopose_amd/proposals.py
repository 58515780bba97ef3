"""Label class-agnostic mask proposals against the template banks: which onboarded object a mask is, and how sure.

A segmenter (SAM, FastSAM, a depth clusterer: anything that emits COCO-RLE masks; the depth clusterer of `depth_proposals` is the project's own) gives the
proposals; `label_proposals` turns them into the CNOS-shaped detection records that `pipeline.infer_detections` and
`provider.test_batch.assemble_test_image` read, from the `tem_rgb` that `onboard_objects` already produced.

The algorithm is the matching stage of CNOS (Nguyen et al., "CNOS: A Strong Baseline for CAD-based Novel Object Segmentation",
2023) WRITTEN FROM ITS PUBLISHED DESCRIPTION, NOT FROM ITS CODE: DINOv2 cls-token descriptors (`x_norm_clstoken`) of the masked
crops, cosine similarity to every template of every object, the mean of the top-k templates per object ("avg_5"), arg-max over
objects, a confidence cut, a cap on the detection count, per-object mask NMS.  Parity with CNOS's own code is unpinned; the
defaults below are CNOS's as remembered.  Its later appearance and geometric scores and box NMS are not here.

The kernels are in csrc/pp_proposals.hip (include/picopose_hip.h, PROPOSAL LABELLING, states each): every dot product is one
fixed summation tree, so the tie rules (lowest view, lowest object) are exact.  tests/proposal_oracle.py restates everything in
numpy float64."""
import numpy as np
import torch

from . import _lib, ops
from .masks import RunTable, check_frame, check_window, rle_area_extent, rle_counts, run_ends
from .provider.test_batch import _frame_u8, detection_window

NORM_EPS = 1e-12        # pp_descriptor_normalize's floor on the norm
LN_EPS = 1e-6           # DINOv2's LayerNorm


def cls_descriptors(net, rgb, bs=16):
    """rgb (n, 3, S, S) normalised crops on the device -> (n, C) fp32: the cls row of the ViT's last block passed through the ViT's
    final `norm` (DINOv2's `x_norm_clstoken`, the descriptor CNOS matches), in mini-batches of `bs` under no_grad and under the
    model's arithmetic mode (`net.precision`).  The `norm` parameters are in every checkpoint; no other path reads them."""
    fe = net.feature_extractor
    norm = fe.dinov2.norm
    out = []
    with torch.no_grad(), ops.precision_scope(getattr(net, "precision", None)):
        for s in range(0, rgb.shape[0], bs):
            cls = fe.forward_tokens(rgb[s:s + bs].contiguous())[0][-1][:, 0].contiguous()
            out.append(ops.layernorm(cls, norm.weight, norm.bias, LN_EPS))
    return torch.cat(out) if out else torch.empty((0, fe.num_features), dtype=torch.float32, device=rgb.device)


def normalize_descriptors(x):
    """(n, C) fp32 on the device -> the rows divided by max(their 2-norm, 1e-12) (pp_descriptor_normalize)."""
    (x,) = _lib.dev_f32(x)
    y = torch.empty_like(x)
    if x.shape[0]:
        _lib.call("pp_descriptor_normalize", x, x.shape[0], x.shape[1], NORM_EPS, y)
    return y


class DescriptorBank:
    """The unit template descriptors of the onboarded objects: `rows` (sum T, C) fp32 on the device, object o owning the rows
    offsets[o] .. offsets[o + 1] (`offsets`: int32 on the device, `offsets_host`: the numpy copy), and `obj_ids[o]` its object id.
    from_rows normalises raw descriptors, `counts` templates per object."""

    def __init__(self, rows, offsets_host, obj_ids):
        offsets_host = np.ascontiguousarray(offsets_host, dtype=np.int32)
        if rows.dim() != 2 or offsets_host.ndim != 1 or len(offsets_host) != len(obj_ids) + 1 or len(obj_ids) == 0:
            raise ValueError("a bank needs rows (sum T, C), one id per object and len(obj_ids) + 1 offsets")
        if offsets_host[0] != 0 or offsets_host[-1] != rows.shape[0] or np.any(np.diff(offsets_host) <= 0):
            raise ValueError("offsets must start at 0, end at the number of rows and leave no object empty")
        self.rows, self.offsets_host, self.obj_ids = rows, offsets_host, [int(i) for i in obj_ids]
        self.offsets = torch.from_numpy(offsets_host).to(rows.device)

    @classmethod
    def from_rows(cls, raw, counts, obj_ids):
        return cls(normalize_descriptors(raw), np.concatenate(([0], np.cumsum(np.asarray(counts, np.int64)))), obj_ids)


def describe_templates(net, templates_data, obj_ids, views=None, bs=16):
    """The DescriptorBank of `templates_data["tem_rgb"]` (O, V, 3, S, S) as onboard_objects returns it, obj_ids[o] the id of object
    o.  views: an optional subset of the V view indices (CNOS matches 42 of its 162 views); view numbers reported by the match
    then count within that subset."""
    tem = templates_data["tem_rgb"]
    if tem.dim() != 5 or tem.shape[0] != len(obj_ids):
        raise ValueError(f"tem_rgb must be (n_objects, V, 3, S, S) with one id per object, got {tuple(tem.shape)} and {len(obj_ids)} ids")
    if views is not None:
        tem = tem[:, torch.as_tensor(np.asarray(views, np.int64), device=tem.device)]
    O, V = tem.shape[:2]
    if V == 0:
        raise ValueError("no template views")
    return DescriptorBank.from_rows(cls_descriptors(net, tem.reshape(O * V, *tem.shape[2:]), bs), [V] * O, obj_ids)


def match_descriptors(query, bank, topk=5):
    """query (P, C) raw descriptors on the device -> (score (P, O) fp32, view (P, O) int32, label (P,) int32, best (P,) fp32) of
    pp_proposal_match: the query is normalised first; score = the mean of the min(topk, T_o) largest cosines to object o's
    templates, view = the template of the largest cosine (lowest on a tie), label = the arg-max over objects (lowest on a tie),
    best = that score.  Nothing waits for the device."""
    q = normalize_descriptors(query)
    P, C = q.shape
    O = len(bank.obj_ids)
    if C != bank.rows.shape[1]:
        raise ValueError(f"query descriptors have {C} channels, the bank {bank.rows.shape[1]}")
    dev = q.device
    score = torch.empty((P, O), dtype=torch.float32, device=dev)
    view = torch.empty((P, O), dtype=torch.int32, device=dev)
    label = torch.empty((P,), dtype=torch.int32, device=dev)
    best = torch.empty((P,), dtype=torch.float32, device=dev)
    if P:
        _lib.call("pp_proposal_match", q, P, bank.rows, bank.offsets, bank.offsets_host, O, C, int(topk), score, view, label, best)
    return score, view, label, best


def mask_intersections(bits):
    """bits (n, words) int32 as `masks.RunTable.pack` writes them -> inter (n, n) int32 on the device, inter[i][j] the pixels masks i
    and j share (pp_mask_intersections)."""
    n, words = bits.shape
    inter = torch.empty((n, n), dtype=torch.int32, device=bits.device)
    _lib.call("pp_mask_intersections", bits, n, words, inter)
    return inter


def _overlaps_of_runs(runs, hw, device):
    bits, area = RunTable.upload(runs, device).pack(hw)
    return mask_intersections(bits), area, bits


def mask_overlaps(segmentations, size, device="cuda"):
    """COCO-RLE masks (any form `rle_counts` accepts) of one (H, W) = size frame -> (inter (n, n) int32, area (n,) int32) on the
    device: inter[i][j] the pixels masks i and j share, its diagonal the areas.  The run lengths are decoded on the host, the
    masks are bit-packed and intersected on the device (pp_rle_pack_bits, pp_mask_intersections); no dense mask is built."""
    H, W = (int(v) for v in size)
    runs = []
    for i, seg in enumerate(segmentations):
        runs.append(run_ends(rle_counts(seg, i, "mask", (H, W))))
    if not runs:
        raise ValueError("no masks")
    check_frame(H, W)
    return _overlaps_of_runs(runs, H * W, device)[:2]


def nms_masks(scores, labels, inter, area, iou, per_object=True):
    """Greedy mask NMS on the host -> the kept indices, best first.  Proposals are visited in descending score, the lower index
    first among equal scores; one is dropped when an earlier KEPT one (per_object: with the same label) overlaps it with
    inter / (area_i + area_j - inter) > iou, the quotient in float64 (an IoU exactly at the threshold is kept)."""
    host = lambda a, dt: (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(dt)  # noqa: E731
    scores, labels, inter, area = host(scores, np.float64), host(labels, np.int64), host(inter, np.int64), host(area, np.int64)
    kept = []
    for i in np.argsort(-scores, kind="stable"):
        for j in kept:
            if per_object and labels[i] != labels[j]:
                continue
            union = area[i] + area[j] - inter[i, j]
            if union > 0 and np.float64(inter[i, j]) / np.float64(union) > iou:
                break
        else:
            kept.append(int(i))
    return kept


def _crop(frame, runs, windows, S, rgb_mask_flag, device):
    """One pp_detections_crop launch: the proposals' crops (n, 3, S, S), resized and CLIP-normalised."""
    n = len(runs)
    table = RunTable.upload(runs, device)
    window = np.ascontiguousarray(windows, dtype=np.int32)
    frame_d = torch.from_numpy(np.ascontiguousarray(frame)).to(device)
    win_d = torch.from_numpy(window.ravel()).to(device)
    rgb = torch.empty((n, 3, S, S), dtype=torch.float32, device=device)
    mask = torch.empty((n, S, S), dtype=torch.float32, device=device)
    table.crop(frame_d, win_d, window, S, rgb_mask_flag, rgb, mask)
    return rgb


def label_proposals(net, image_u8, proposals, bank, *, scene_id, img_id, topk=5, min_score=0.5, max_detections=100, nms_iou=0.25,
                    min_area_px=0, rgb_mask_flag=True, img_size=224, minimum_n_point=8, bs=16, time=0.0, device="cuda", timings=None):
    """One decoded image and a segmenter's mask proposals -> CNOS-shaped detection records, best first.
    proposals: dicts with `segmentation` (COCO RLE, any form `rle_counts` accepts) and optionally `bbox` [x, y, w, h] (default: the
    mask's box; it only matters for masks of at most `minimum_n_point` pixels, as in `detection_window`).  bank: describe_templates'.
    In this order: the proposals are parsed (ValueError names the proposal); masks of area <= min_area_px are dropped (an empty
    mask always is); one pp_detections_crop launch crops the windows of `detection_window` (rgb_mask_flag: background zeroed, as
    CNOS does); cls_descriptors; match_descriptors; proposals with best > min_score are kept, then the `max_detections` best
    (the lower index first among equal scores); mask_overlaps on the survivors only; nms_masks (per object, IoU > nms_iou).
    Each record: scene_id, image_id, category_id (= bank.obj_ids[label]), bbox [x, y, w, h] of the mask, score, time, segmentation
    (the proposal's own) and view (the best template of that object, counted within the bank).  `assemble_test_image` and
    `pipeline.infer_detections` take the list as it is; an empty list is a valid result.
    The defaults are CNOS's as remembered (avg_5, confidence 0.5, 100 detections, NMS 0.25, masked crops), not read from its code.
    timings: a dict that receives the wall-clock seconds of crop, vit, match, overlaps and host (each section then ends with a
    device synchronisation; None: no extra waits — the call waits once, for the scores)."""
    import time as _time

    frame = _frame_u8(image_u8)
    H, W = frame.shape[:2]
    check_frame(H, W)
    tick = [_time.perf_counter()]

    def lap(name):
        if timings is not None:
            torch.cuda.synchronize()
            now = _time.perf_counter()
            timings[name] = timings.get(name, 0.0) + now - tick[0]
            tick[0] = now

    idx, runs, boxes, windows = [], [], [], []
    for i, prop in enumerate(proposals):
        try:
            seg = prop["segmentation"]
        except (KeyError, TypeError):
            raise ValueError(f"proposal {i}: a proposal is a dict with a 'segmentation'") from None
        counts = rle_counts(seg, i, "proposal", (H, W))
        area, extent = rle_area_extent(counts, H)
        if area <= min_area_px or extent is None:
            continue
        rmin, rmax, cmin, cmax = extent
        box = [cmin, rmin, cmax - cmin + 1, rmax - rmin + 1]
        _, win = detection_window(counts, (H, W), prop.get("bbox", box), minimum_n_point)
        check_window(win, H, W, i, "proposal")
        idx.append(i)
        runs.append(run_ends(counts))
        boxes.append(box)
        windows.append(win)
    lap("host")
    if not idx:
        return []
    rgb = _crop(frame, runs, windows, int(img_size), rgb_mask_flag, device)
    lap("crop")
    desc = cls_descriptors(net, rgb, bs)
    lap("vit")
    _, view, label, best = match_descriptors(desc, bank, topk)
    view_of = view.gather(1, label.long()[:, None])[:, 0]
    best_h, label_h, view_h = best.cpu().numpy(), label.cpu().numpy(), view_of.cpu().numpy()
    lap("match")
    order = np.argsort(-best_h.astype(np.float64), kind="stable")
    cand = [int(k) for k in order if best_h[k] > min_score][:int(max_detections)]
    lap("host")
    if not cand:
        return []
    inter, area, _ = _overlaps_of_runs([runs[k] for k in cand], H * W, device)
    inter_h, area_h = inter.cpu().numpy(), area.cpu().numpy()
    lap("overlaps")
    kept = [cand[k] for k in nms_masks(best_h[cand], label_h[cand], inter_h, area_h, nms_iou, per_object=True)]
    records = [{"scene_id": int(scene_id), "image_id": int(img_id), "category_id": bank.obj_ids[int(label_h[k])], "bbox": boxes[k],
                "score": float(best_h[k]), "time": float(time), "segmentation": proposals[idx[k]]["segmentation"], "view": int(view_h[k])}
               for k in kept]
    lap("host")
    return records
