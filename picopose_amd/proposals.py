"""Label class-agnostic mask proposals against the template banks: which onboarded object a mask is, and how sure.

A segmenter (SAM, FastSAM, a depth clusterer: anything that emits COCO-RLE masks; the depth clusterer of `depth_proposals` is the project's own) gives the
proposals; `label_proposals` turns them into the CNOS-shaped detection records that `pipeline.infer_detections` and
`provider.test_batch.assemble_test_image` read, from the `tem_rgb` that `onboard_objects` already produced.

The algorithm is the matching stage of CNOS (Nguyen et al., "CNOS: A Strong Baseline for CAD-based Novel Object Segmentation",
2023) WRITTEN FROM ITS PUBLISHED DESCRIPTION, NOT FROM ITS CODE: DINOv2 cls-token descriptors (`x_norm_clstoken`) of the masked
crops, cosine similarity to every template of every object, the mean of the top-k templates per object ("avg_5"), arg-max over
objects, a confidence cut, a cap on the detection count, per-object mask NMS.  Parity with CNOS's own code is unpinned; the
defaults below are CNOS's as remembered.

Opt-in (`label_proposals(appearance=True)` on a bank built with `describe_templates(patches=True)`): the APPEARANCE SCORE of the
instance-segmentation stage of SAM-6D (Lin et al., 2024), CNOS's published successor, again WRITTEN FROM ITS PUBLISHED DESCRIPTION,
NOT FROM ITS CODE: from the patch tokens of the same ViT pass, for every foreground patch of the crop the best cosine to any
foreground patch of the best-matching template, averaged over the crop's foreground patches; the detection score becomes
(semantic + w appearance) / (1 + w).  Parity with SAM-6D's code is unpinned, the default weight of 1 is untuned, and the effect on
real data is unmeasured (`detection_eval` and `pose_detection_eval` are the tools to measure it with).  SAM-6D's geometric score
and box NMS are not here.

The kernels are in csrc/pp_proposals.hip and csrc/pp_appearance.hip (include/picopose_hip.h, PROPOSAL LABELLING, states each): every
dot product is one fixed summation order, so the tie rules (lowest view, lowest object, lowest patch) are exact.
tests/proposal_oracle.py and tests/appearance_oracle.py restate everything in numpy float64."""
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


def token_descriptors(net, rgb, bs=16):
    """rgb (n, 3, S, S) -> (cls (n, C), patches (n, N, C)) fp32 from ONE ViT pass per mini-batch, both through the ViT's final `norm`
    (DINOv2's `x_norm_clstoken` and `x_norm_patchtokens`); patch i = py * (S / patch) + px, the ViT's token order.  The cls half
    is made by the launches of `cls_descriptors` (the cls rows made contiguous, the same layer-norm call): same bits for the same bs."""
    fe = net.feature_extractor
    norm = fe.dinov2.norm
    C = fe.num_features
    N = (rgb.shape[2] // fe.patch_size) * (rgb.shape[3] // fe.patch_size)
    out_c, out_p = [], []
    with torch.no_grad(), ops.precision_scope(getattr(net, "precision", None)):
        for s in range(0, rgb.shape[0], bs):
            tok = fe.forward_tokens(rgb[s:s + bs].contiguous())[0][-1]
            out_c.append(ops.layernorm(tok[:, 0].contiguous(), norm.weight, norm.bias, LN_EPS))
            rows = tok[:, 1:].contiguous().view(tok.shape[0] * N, C)
            out_p.append(ops.layernorm(rows, norm.weight, norm.bias, LN_EPS).view(tok.shape[0], N, C))
    if not out_c:
        return (torch.empty((0, C), dtype=torch.float32, device=rgb.device), torch.empty((0, N, C), dtype=torch.float32, device=rgb.device))
    return torch.cat(out_c), torch.cat(out_p)


def patch_valid(mask, patch):
    """mask (n, S, S) fp32 on the device (a crop's resized mask, or a `tem_mask`), S a multiple of `patch` -> (valid (n, N) uint8,
    n_valid (n,) int32) of pp_patch_valid: patch i = py * (S / patch) + px is valid iff at least half of its patch x patch pixels
    have mask > 0.5."""
    (mask,) = _lib.dev_f32(mask)
    if mask.dim() != 3 or mask.shape[1] != mask.shape[2] or patch <= 0 or mask.shape[1] % patch:
        raise ValueError(f"masks must be (n, S, S) with S a multiple of the patch size {patch}, got {tuple(mask.shape)}")
    n, S = mask.shape[:2]
    valid = torch.empty((n, (S // patch) ** 2), dtype=torch.uint8, device=mask.device)
    n_valid = torch.empty((n,), dtype=torch.int32, device=mask.device)
    if n:
        _lib.call("pp_patch_valid", mask, n, S, int(patch), valid, n_valid)
    return valid, n_valid


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
    from_rows normalises raw descriptors, `counts` templates per object.
    Optional, for the appearance score (describe_templates(patches=True)): `patch_rows` (sum T, N, C) fp32, the unit patch
    descriptors of every template in the ViT's token order, and `patch_valid` (sum T, N) uint8, its foreground patches; both None
    on a bank without them."""

    def __init__(self, rows, offsets_host, obj_ids, patch_rows=None, patch_valid=None):
        offsets_host = np.ascontiguousarray(offsets_host, dtype=np.int32)
        if rows.dim() != 2 or offsets_host.ndim != 1 or len(offsets_host) != len(obj_ids) + 1 or len(obj_ids) == 0:
            raise ValueError("a bank needs rows (sum T, C), one id per object and len(obj_ids) + 1 offsets")
        if offsets_host[0] != 0 or offsets_host[-1] != rows.shape[0] or np.any(np.diff(offsets_host) <= 0):
            raise ValueError("offsets must start at 0, end at the number of rows and leave no object empty")
        self.rows, self.offsets_host, self.obj_ids = rows, offsets_host, [int(i) for i in obj_ids]
        self.offsets = torch.from_numpy(offsets_host).to(rows.device)
        if (patch_rows is None) != (patch_valid is None):
            raise ValueError("a bank carries patch_rows and patch_valid together or neither")
        if patch_rows is not None and (patch_rows.dim() != 3 or patch_rows.shape[0] != rows.shape[0] or patch_rows.shape[2] != rows.shape[1]
                                       or tuple(patch_valid.shape) != tuple(patch_rows.shape[:2]) or patch_valid.dtype != torch.uint8):
            raise ValueError("patch_rows must be (sum T, N, C) next to rows (sum T, C), patch_valid (sum T, N) uint8")
        if patch_rows is not None and not (patch_rows.device == patch_valid.device == rows.device):
            raise ValueError(f"patch_rows ({patch_rows.device}) and patch_valid ({patch_valid.device}) must be on the device of rows ({rows.device})")
        self.patch_rows, self.patch_valid = patch_rows, patch_valid

    @classmethod
    def from_rows(cls, raw, counts, obj_ids, patch_raw=None, patch_valid=None):
        """patch_raw (sum T, N, C): raw patch tokens, normalised row by row like `raw`."""
        patch_rows = None if patch_raw is None else normalize_descriptors(patch_raw.reshape(-1, patch_raw.shape[-1])).view(patch_raw.shape)
        return cls(normalize_descriptors(raw), np.concatenate(([0], np.cumsum(np.asarray(counts, np.int64)))), obj_ids, patch_rows, patch_valid)


def describe_templates(net, templates_data, obj_ids, views=None, bs=16, patches=False):
    """The DescriptorBank of `templates_data["tem_rgb"]` (O, V, 3, S, S) as onboard_objects returns it, obj_ids[o] the id of object
    o.  views: an optional subset of the V view indices (CNOS matches 42 of its 162 views); view numbers reported by the match
    then count within that subset.
    patches=True: the bank also carries `patch_rows` (the unit patch tokens of the same ViT pass) and `patch_valid` (from
    `templates_data["tem_mask"]` (O, V, S, S), the same `views`; ValueError without it), which the appearance score reads.  They
    are fp32 on the device: V * N * C * 4 bytes per object, 42 views x 256 patches x 1024 channels = 44 MB, 1.3 GB for 30 objects."""
    tem = templates_data["tem_rgb"]
    if tem.dim() != 5 or tem.shape[0] != len(obj_ids):
        raise ValueError(f"tem_rgb must be (n_objects, V, 3, S, S) with one id per object, got {tuple(tem.shape)} and {len(obj_ids)} ids")
    mask = None
    if patches:
        mask = templates_data.get("tem_mask")
        if mask is None:
            raise ValueError("patches=True needs templates_data['tem_mask']")
        if tuple(mask.shape) != (*tem.shape[:2], *tem.shape[3:]):
            raise ValueError(f"tem_mask must be (n_objects, V, S, S) like tem_rgb, got {tuple(mask.shape)}")
    if views is not None:
        pick = torch.as_tensor(np.asarray(views, np.int64), device=tem.device)
        tem = tem[:, pick]
        mask = mask[:, pick.to(mask.device)] if patches else None
    O, V = tem.shape[:2]
    if V == 0:
        raise ValueError("no template views")
    rgb = tem.reshape(O * V, *tem.shape[2:])
    if not patches:
        return DescriptorBank.from_rows(cls_descriptors(net, rgb, bs), [V] * O, obj_ids)
    cls, tokens = token_descriptors(net, rgb, bs)
    valid, _ = patch_valid(mask.reshape(O * V, *mask.shape[2:]).to(rgb.device), net.feature_extractor.patch_size)
    return DescriptorBank.from_rows(cls, [V] * O, obj_ids, tokens, valid)


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


def appearance_scores(q_patches, q_valid, bank, rows):
    """q_patches (P, N, C) raw patch tokens on the device, q_valid (P, N) uint8 (patch_valid's), rows: P bank rows (host integers,
    the template view each proposal is compared with) -> (app (P,) fp32, patch_sim (P, N) fp32, patch_arg (P, N) int32,
    n_valid (P,) int32) of pp_appearance_match: the tokens are normalised first; patch_sim = the largest cosine of every query patch
    to the valid patches of its view and patch_arg that patch (the lowest among equals; 0 and -1 for a view without a valid patch),
    app = the mean of patch_sim over the valid query patches (0 without one).  Nothing waits for the device."""
    if bank.patch_rows is None:
        raise ValueError("the bank carries no patch descriptors: build it with describe_templates(..., patches=True)")
    dev = bank.patch_rows.device
    if not (dev.type == "cuda" and q_patches.device == q_valid.device == bank.patch_valid.device == dev):
        raise ValueError(f"the query patch tokens ({q_patches.device}), q_valid ({q_valid.device}) and the bank's patches ({dev}) must be on one GPU")
    (q_patches,) = _lib.dev_f32(q_patches)
    R, N, C = bank.patch_rows.shape
    if q_patches.dim() != 3 or tuple(q_patches.shape[1:]) != (N, C):
        raise ValueError(f"query patch tokens must be (P, {N}, {C}) like the bank's, got {tuple(q_patches.shape)}")
    P = q_patches.shape[0]
    q_valid = q_valid.contiguous()
    if tuple(q_valid.shape) != (P, N) or q_valid.dtype != torch.uint8:
        raise ValueError(f"q_valid must be ({P}, {N}) uint8, got {tuple(q_valid.shape)} {q_valid.dtype}")
    rows_host = np.ascontiguousarray(rows, dtype=np.int32)
    if rows_host.shape != (P,) or (P and (rows_host.min() < 0 or rows_host.max() >= R)):
        raise ValueError(f"rows must be {P} bank rows in [0, {R})")
    dev = q_patches.device
    app = torch.empty((P,), dtype=torch.float32, device=dev)
    patch_sim = torch.empty((P, N), dtype=torch.float32, device=dev)
    patch_arg = torch.empty((P, N), dtype=torch.int32, device=dev)
    n_valid = torch.empty((P,), dtype=torch.int32, device=dev)
    if P:
        q = normalize_descriptors(q_patches.view(P * N, C))
        _lib.call("pp_appearance_match", q, q_valid, P, bank.patch_rows, bank.patch_valid, R, torch.from_numpy(rows_host).to(dev), rows_host,
                  N, C, patch_sim, patch_arg, n_valid, app)
    return app, patch_sim, patch_arg, n_valid


def combined_scores(semantic, appearance, weight):
    """(semantic + weight * appearance) / (1 + weight) in float64 on the host."""
    return (np.asarray(semantic, np.float64) + float(weight) * np.asarray(appearance, np.float64)) / (1.0 + float(weight))


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
    """One pp_detections_crop launch: the proposals' crops (n, 3, S, S), resized and CLIP-normalised, and their resized masks (n, S, S)."""
    n = len(runs)
    table = RunTable.upload(runs, device)
    window = np.ascontiguousarray(windows, dtype=np.int32)
    frame_d = torch.from_numpy(np.ascontiguousarray(frame)).to(device)
    win_d = torch.from_numpy(window.ravel()).to(device)
    rgb = torch.empty((n, 3, S, S), dtype=torch.float32, device=device)
    mask = torch.empty((n, S, S), dtype=torch.float32, device=device)
    table.crop(frame_d, win_d, window, S, rgb_mask_flag, rgb, mask)
    return rgb, mask


def label_proposals(net, image_u8, proposals, bank, *, scene_id, img_id, topk=5, min_score=0.5, max_detections=100, nms_iou=0.25,
                    min_area_px=0, rgb_mask_flag=True, img_size=224, minimum_n_point=8, bs=16, time=0.0, device="cuda", timings=None,
                    appearance=False, appearance_weight=1.0):
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
    device synchronisation; None: no extra waits — the call waits once, for the scores), and of appearance with appearance=True.
    appearance=True (bank: describe_templates(..., patches=True), ValueError otherwise; appearance_weight w >= 0): everything up to
    and including the confidence cut and the cap runs on the semantic (cls) score as above.  For the survivors only, the patch
    tokens of the same ViT pass (token_descriptors), with the crop's resized mask deciding their foreground patches
    (patch_valid), are compared with bank row offsets_host[label] + view, the best template of the chosen object
    (appearance_scores); score = (semantic + w appearance) / (1 + w) in float64 on the host; the NMS visits the survivors in
    descending combined score, the lower proposal index first among equals, and the records come out in that order with two more
    keys, semantic_score and appearance_score.  This is SAM-6D's appearance term from its published description; the weight of 1
    is untuned and the effect on real data unmeasured.  With appearance=False nothing of this runs and no record has the keys."""
    import time as _time

    if appearance:
        if bank.patch_rows is None:
            raise ValueError("appearance=True needs a bank with patch descriptors: describe_templates(..., patches=True)")
        if not float(appearance_weight) >= 0.0 or not np.isfinite(float(appearance_weight)):
            raise ValueError(f"appearance_weight must be finite and >= 0, got {appearance_weight}")
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
    rgb, crop_mask = _crop(frame, runs, windows, int(img_size), rgb_mask_flag, device)
    lap("crop")
    if appearance:
        desc, tokens = token_descriptors(net, rgb, bs)
    else:
        del crop_mask
        desc = cls_descriptors(net, rgb, bs)
    lap("vit")
    _, view, label, best = match_descriptors(desc, bank, topk)
    view_of = view.gather(1, label.long()[:, None])[:, 0]
    best_h, label_h, view_h = best.cpu().numpy(), label.cpu().numpy(), view_of.cpu().numpy()
    lap("match")
    order = np.argsort(-best_h.astype(np.float64), kind="stable")
    cand = [int(k) for k in order if best_h[k] > min_score][:int(max_detections)]
    if appearance:
        cand.sort()                     # ascending proposal index: the NMS's "lower index first among equal scores"
    lap("host")
    if not cand:
        return []
    score_h = best_h
    if appearance:
        pick = torch.as_tensor(cand, dtype=torch.long, device=tokens.device)
        q_valid, _ = patch_valid(crop_mask[pick], net.feature_extractor.patch_size)
        rows = bank.offsets_host[label_h[cand]].astype(np.int64) + view_h[cand]
        app_h = np.zeros(len(idx), np.float32)
        app_h[cand] = appearance_scores(tokens[pick], q_valid, bank, rows)[0].cpu().numpy()
        score_h = combined_scores(best_h, app_h, appearance_weight)
        del tokens, crop_mask
        lap("appearance")
    inter, area, _ = _overlaps_of_runs([runs[k] for k in cand], H * W, device)
    inter_h, area_h = inter.cpu().numpy(), area.cpu().numpy()
    lap("overlaps")
    kept = [cand[k] for k in nms_masks(score_h[cand], label_h[cand], inter_h, area_h, nms_iou, per_object=True)]
    records = [{"scene_id": int(scene_id), "image_id": int(img_id), "category_id": bank.obj_ids[int(label_h[k])], "bbox": boxes[k],
                "score": float(score_h[k]), "time": float(time), "segmentation": proposals[idx[k]]["segmentation"], "view": int(view_h[k])}
               for k in kept]
    if appearance:
        for r, k in zip(records, kept):
            r["semantic_score"], r["appearance_score"] = float(best_h[k]), float(app_h[k])
    lap("host")
    return records
