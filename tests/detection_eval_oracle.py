"""numpy restatement of DETECTION SCORING (include/picopose_hip.h) in literal loops: grouping and ordering, the overlaps from DENSE
masks and from boxes, the greedy matching as the SEQUENTIAL scan over the materialised group order (pp_det_match computes the closed
form: the two formulations check each other), accumulation and the twelve summary numbers.  `match` returns the tables in the layout
of picopose_amd.detection_eval.match_detections, so a test compares key by key.  Also the seeded cases both test files share."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detections_oracle as do  # noqa: E402

IOU_THRS = np.linspace(.5, .95, 10)
AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
MAX_DETS = (1, 10, 100)
NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
TABLES = ("inter", "iou", "dt_match", "dt_ignore", "gt_match", "gt_ignore")
LAYOUT = ("group_image", "group_category", "group_det", "group_gt", "group_pair", "det_index", "gt_index", "det_score")


def group_records(detections, annotations, max_dets=MAX_DETS, class_agnostic=False):
    """-> (images, categories, groups): the sorted image keys and category ids, and one (image index, category index, detection
    indices sorted by descending score — stably — and cut to max(max_dets), annotation indices in input order) per (image, category)
    that holds a record, sorted by (image, category)."""
    cat = (lambda r: 0) if class_agnostic else (lambda r: int(r["category_id"]))
    key = lambda r: (int(r["scene_id"]), int(r["image_id"]))  # noqa: E731
    images = sorted({key(r) for r in list(detections) + list(annotations)})
    cats = sorted({cat(r) for r in list(detections) + list(annotations)})
    groups = []
    for i, im in enumerate(images):
        for k, c in enumerate(cats):
            d = [n for n, r in enumerate(detections) if key(r) == im and cat(r) == c]
            g = [n for n, r in enumerate(annotations) if key(r) == im and cat(r) == c]
            if not d and not g:
                continue
            d = sorted(d, key=lambda n: -float(detections[n]["score"]))[:max(max_dets)]       # sorted() is stable
            groups.append((i, k, d, g))
    return images, cats, groups


def overlaps(dets, gts, iou_type):
    """The D x G block of one group -> (inter int32 or None, iou float64), pair by pair."""
    D, G = len(dets), len(gts)
    inter, iou = np.zeros((D, G), np.int32), np.zeros((D, G), np.float64)
    if iou_type == "segm":
        dm, gm = [do.decode(r["segmentation"]) > 0 for r in dets], [do.decode(r["segmentation"]) > 0 for r in gts]
    for i in range(D):
        for j in range(G):
            crowd = bool(gts[j].get("iscrowd", False))
            if iou_type == "segm":
                n = int(np.logical_and(dm[i], gm[j]).sum())
                ad, ag = int(dm[i].sum()), int(gm[j].sum())
                den = ad if crowd else ad + ag - n
                inter[i, j] = n
                iou[i, j] = np.float64(n) / np.float64(den) if den > 0 else 0.0
            else:
                xd, yd, wd, hd = (np.float64(v) for v in dets[i]["bbox"])
                xg, yg, wg, hg = (np.float64(v) for v in gts[j]["bbox"])
                iw = max(np.float64(0), min(xd + wd, xg + wg) - max(xd, xg))
                ih = max(np.float64(0), min(yd + hd, yg + hg) - max(yd, yg))
                num = iw * ih
                den = wd * hd if crowd else (wd * hd + wg * hg) - num
                iou[i, j] = num / den if den > 0 else 0.0
    return (inter if iou_type == "segm" else None), iou


def match_group(iou, gt_flag, gt_crowd, gt_area, det_area, lo, hi, thr):
    """The sequential scan for one group, area range and threshold -> (dtm, dtig, gtm, gtig), indices within the group in INPUT order."""
    D, G = iou.shape
    gig = [bool(gt_flag[j]) or gt_area[j] < lo or gt_area[j] > hi for j in range(G)]
    order = [j for j in range(G) if not gig[j]] + [j for j in range(G) if gig[j]]
    gtm, dtm, dtig = [-1] * G, [-1] * D, [False] * D
    for d in range(D):
        best, m = min(thr, 1 - 1e-10), -1
        for j in order:
            if gtm[j] >= 0 and not gt_crowd[j]:
                continue
            if m >= 0 and not gig[m] and gig[j]:
                break
            if iou[d, j] < best:
                continue
            best, m = iou[d, j], j
        if m >= 0:
            dtm[d], dtig[d], gtm[m] = m, gig[m], d
        else:
            dtig[d] = bool(det_area[d] < lo or det_area[d] > hi)
    return dtm, dtig, gtm, gig


def mask_area(record):
    return int((do.decode(record["segmentation"]) > 0).sum())


def match(detections, annotations, iou_type="segm", iou_thrs=None, area_ranges=None, max_dets=MAX_DETS, class_agnostic=False,
          match_group=match_group):
    thrs = np.asarray(IOU_THRS if iou_thrs is None else iou_thrs, np.float64)
    ranges = np.asarray(AREA_RANGES if area_ranges is None else area_ranges, np.float64).reshape(-1, 2)
    images, cats, groups = group_records(detections, annotations, max_dets, class_agnostic)
    A, T = len(ranges), len(thrs)
    n_det, n_gt = sum(len(g[2]) for g in groups), sum(len(g[3]) for g in groups)
    out = {"iou_type": iou_type, "iou_thrs": thrs, "area_ranges": ranges, "max_dets": tuple(max_dets), "images": images, "categories": cats,
           "dt_match": np.full((A, T, n_det), -1, np.int32), "dt_ignore": np.zeros((A, T, n_det), np.uint8),
           "gt_match": np.full((A, T, n_gt), -1, np.int32), "gt_ignore": np.zeros((A, n_gt), np.uint8)}
    gi, gc, gd, gg, gp, di, gx, inter, iou = [], [], [], [], [], [], [], [], []
    d0 = g0 = p0 = 0
    for i, k, d, g in groups:
        dets, gts = [detections[n] for n in d], [annotations[n] for n in g]
        bi, bo = overlaps(dets, gts, iou_type)
        flag = [bool(r.get("ignore", False)) or bool(r.get("iscrowd", False)) for r in gts]
        crowd = [bool(r.get("iscrowd", False)) for r in gts]
        garea = [np.float64(mask_area(r)) for r in gts]
        darea = [np.float64(mask_area(r)) if iou_type == "segm" else np.float64(r["bbox"][2]) * np.float64(r["bbox"][3]) for r in dets]
        for a in range(A):
            for t in range(T):
                dtm, dtig, gtm, gig = match_group(bo, flag, crowd, garea, darea, ranges[a, 0], ranges[a, 1], thrs[t])
                out["dt_match"][a, t, d0:d0 + len(d)] = [g0 + m if m >= 0 else -1 for m in dtm]
                out["dt_ignore"][a, t, d0:d0 + len(d)] = dtig
                out["gt_match"][a, t, g0:g0 + len(g)] = [d0 + m if m >= 0 else -1 for m in gtm]
                out["gt_ignore"][a, g0:g0 + len(g)] = gig
        gi.append(i), gc.append(k), gd.append((d0, len(d))), gg.append((g0, len(g))), gp.append(p0)
        di += d
        gx += g
        iou.append(bo.ravel())
        if bi is not None:
            inter.append(bi.ravel())
        d0, g0, p0 = d0 + len(d), g0 + len(g), p0 + len(d) * len(g)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)  # noqa: E731
    out.update(group_image=np.array(gi, np.int64), group_category=np.array(gc, np.int64), group_det=np.array(gd, np.int64).reshape(-1, 2),
               group_gt=np.array(gg, np.int64).reshape(-1, 2), group_pair=np.array(gp, np.int64), det_index=np.array(di, np.int64),
               gt_index=np.array(gx, np.int64), det_score=np.array([float(detections[n]["score"]) for n in di], np.float64),
               inter=cat(inter, np.int32) if iou_type == "segm" else None, iou=cat(iou, np.float64))
    return out


def accumulate(m):
    thrs, ranges, max_dets, cats = m["iou_thrs"], m["area_ranges"], m["max_dets"], m["categories"]
    T, A, M, K = len(thrs), len(ranges), len(max_dets), len(cats)
    rec = np.linspace(0, 1, 101)
    precision, recall = -np.ones((T, 101, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        rows = [g for g in range(len(m["group_category"])) if m["group_category"][g] == k]
        for a in range(A):
            npig = 0
            for g in rows:
                s, n = m["group_gt"][g]
                npig += int((m["gt_ignore"][a, s:s + n] == 0).sum())
            if npig == 0:
                continue
            for mi, md in enumerate(max_dets):
                sel = []
                for g in rows:
                    s, n = m["group_det"][g]
                    sel += list(range(s, s + min(n, md)))
                sel = np.array(sel, np.int64)
                sel = sel[np.argsort(-m["det_score"][sel], kind="mergesort")]
                for t in range(T):
                    matched, ign = m["dt_match"][a, t, sel] >= 0, m["dt_ignore"][a, t, sel] != 0
                    tp = np.cumsum(matched & ~ign).astype(np.float64)
                    fp = np.cumsum(~matched & ~ign).astype(np.float64)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, mi] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = np.zeros(101)
                    for r, ind in enumerate(np.searchsorted(rc, rec, side="left")):
                        if ind < nd:
                            q[r] = pr[ind]
                    precision[t, :, k, a, mi] = q
    return {"precision": precision, "recall": recall, "iou_thrs": thrs, "area_ranges": ranges, "max_dets": max_dets, "categories": cats}


def _mean(x):
    x = x[x > -1]
    return float(np.mean(x)) if x.size else -1.0


def summarize(acc):
    """The twelve numbers (area ranges and max_dets read BY POSITION: all, small, medium, large; 1, 10, 100) and per-object AP."""
    p, r, thrs = acc["precision"], acc["recall"], acc["iou_thrs"]
    A, M = p.shape[3], p.shape[4]

    def ap(a, thr=None):
        if a >= A:
            return -1.0
        t = slice(None) if thr is None else np.where(thrs == thr)[0]
        return _mean(p[t, :, :, a, M - 1])

    def ar(a, mi):
        return _mean(r[:, :, a, mi]) if a < A and mi < M else -1.0

    out = dict(zip(NAMES, [ap(0), ap(0, .5), ap(0, .75), ap(1), ap(2), ap(3), ar(0, 0), ar(0, 1), ar(0, 2), ar(1, M - 1), ar(2, M - 1), ar(3, M - 1)]))
    out["per_object_AP"] = {c: _mean(p[:, :, k, 0, M - 1]) for k, c in enumerate(acc["categories"])}
    return out


def score(detections, annotations, **kw):
    return summarize(accumulate(match(detections, annotations, **kw)))


# ---- the closed form (what the kernel computes), restated for the CPU tests -------------------------------------------------------

def match_group_closed(iou, gt_flag, gt_crowd, gt_area, det_area, lo, hi, thr):
    D, G = iou.shape
    gig = np.array([bool(gt_flag[j]) or gt_area[j] < lo or gt_area[j] > hi for j in range(G)], bool)
    crowd = np.asarray(gt_crowd, bool).reshape(G)
    matched = np.zeros(G, bool)
    gtm, dtm, dtig = [-1] * G, [-1] * D, [False] * D
    best0 = min(thr, 1 - 1e-10)
    for d in range(D):
        ok = (~matched | crowd) & (iou[d] >= best0)
        m = -1
        for cls in (~gig, gig):
            c = np.nonzero(ok & cls)[0]
            if c.size:
                m = int(c[iou[d, c] == iou[d, c].max()].max())
                break
        if m >= 0:
            dtm[d], dtig[d], gtm[m], matched[m] = m, bool(gig[m]), d, True
        else:
            dtig[d] = bool(det_area[d] < lo or det_area[d] > hi)
    return dtm, dtig, gtm, list(gig)


# ---- seeded cases shared by the CPU and GPU tests --------------------------------------------------------------------------------

def rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def det(mask, score, cat=1, scene=1, image=1, bbox=None, compressed=False):
    r = do.record(mask, score, cat, compressed=compressed, bbox=bbox if bbox is not None else (_box(mask)))
    r["scene_id"], r["image_id"] = scene, image
    return r


def _box(mask):
    ys, xs = np.nonzero(mask)
    return [0, 0, 0, 0] if ys.size == 0 else [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


def ann(mask, cat=1, scene=1, image=1, ignore=False, iscrowd=False, bbox=None):
    r = det(mask, 0.0, cat, scene, image, bbox)
    del r["score"], r["time"]
    r["ignore"], r["iscrowd"] = bool(ignore), bool(iscrowd)
    return r


SMALL_RANGES = ((0.0, 1e10), (0.0, 16.0), (16.0, 64.0), (64.0, 1e10))


def _rand_mask(rng, H, W):
    kind = rng.integers(0, 8)
    if kind == 0:
        return np.zeros((H, W), np.uint8)                                   # an empty mask
    h, w = int(rng.integers(1, H // 2 + 1)), int(rng.integers(1, W // 2 + 1))
    if kind == 1:
        h, w = 4, 4                                                         # area 16: exactly on an edge of SMALL_RANGES
    if kind == 2:
        h, w = 8, 8                                                         # area 64
    y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
    m = rect(H, W, y, y + h, x, x + w)
    if kind >= 6:
        m &= (rng.random((H, W)) > 0.2).astype(np.uint8)
    return m


def _jitter(rng, mask):
    """A detection near a ground truth: the mask shifted by up to two pixels, or the mask itself."""
    dy, dx = (int(v) for v in rng.integers(-2, 3, 2))
    return np.roll(np.roll(mask, dy, 0), dx, 1) if rng.random() < 0.7 else mask.copy()


def _fbox(rng, mask):
    b = np.asarray(_box(mask), np.float64)
    return [float(v) for v in b + np.concatenate((rng.uniform(-1.5, 1.5, 2), rng.uniform(0, 2.5, 2)))]


def image_case(rng, H, W, scene, image, sides):
    """One image: per category (D, G) = sides[cat].  Ground truths: random masks with duplicates (the last-index tie), a crowd and
    an ignored one AHEAD of non-ignored ones; detections: jittered ground truths and clutter, scores from a short list (equal
    scores), boxes non-integer."""
    dets, anns = [], []
    for cat, (D, G) in sides.items():
        gm = []
        for j in range(G):
            m = gm[j - 1] if j and rng.random() < 0.25 else _rand_mask(rng, H, W)            # a duplicated ground-truth mask
            gm.append(m)
            anns.append(ann(m, cat, scene, image, ignore=(j == 0 and G > 1) or rng.random() < 0.15, iscrowd=(j == 1 and G > 2) or rng.random() < 0.05,
                            bbox=_fbox(rng, m)))
        for i in range(D):
            m = _jitter(rng, gm[int(rng.integers(0, G))]) if G and rng.random() < 0.8 else _rand_mask(rng, H, W)
            dets.append(det(m, float(rng.choice([0.9, 0.8, 0.8, 0.5, 0.25]) if rng.random() < 0.6 else rng.random()), cat, scene, image,
                            bbox=_fbox(rng, m), compressed=bool(i % 2)))
    return dets, anns


@functools.lru_cache(maxsize=None)
def random_case(seed=0, big=True):
    """Two frame sizes in one call (24 x 20: hw = 480, a part-filled last word; 37 x 29), G_g in {0, 1, 3, 64, 65, 130}, D_g in {0, 1, 7,
    100, 101}.  big=False: the small groups only (the CPU tests' closed-form check)."""
    rng = np.random.default_rng(seed)
    plan = [((24, 20), 1, 1, {1: (7, 3), 2: (1, 1), 3: (0, 3), 4: (7, 0)}),
            ((37, 29), 1, 2, {1: (7, 3), 2: (1, 0), 5: (3, 1)}),
            ((24, 20), 2, 1, {1: (3, 3), 2: (7, 1)})]
    if big:
        plan += [((24, 20), 2, 5, {1: (100, 64), 2: (101, 65)}), ((37, 29), 3, 1, {1: (101, 130), 3: (7, 3)}), ((24, 20), 3, 2, {2: (100, 3)})]
    dets, anns = [], []
    for (H, W), scene, image, sides in plan:
        d, a = image_case(rng, H, W, scene, image, sides)
        dets += d
        anns += a
    order = rng.permutation(len(dets))                                       # the input order is not the group order
    return tuple(dets[i] for i in order), tuple(anns)


@functools.lru_cache(maxsize=None)
def threshold_case():
    """IoUs exactly at a threshold, 24 x 20 frame, one category: detection 0 has inter / union = 8 / 16 = 1/2 with ground truth 0 and
    detection 1 has 12 / 16 = 3/4 with ground truth 1; ground truth 2 is a crowd that detections 2 and 3 both match; detection 4 sits on
    two IDENTICAL ground truths 3 and 4 (the last index wins)."""
    H, W = 24, 20
    anns = [ann(rect(H, W, 0, 4, 0, 3)), ann(rect(H, W, 8, 12, 0, 4)), ann(rect(H, W, 14, 22, 8, 16), iscrowd=True),
            ann(rect(H, W, 0, 4, 10, 14)), ann(rect(H, W, 0, 4, 10, 14))]
    dets = [det(rect(H, W, 0, 4, 1, 4), 0.9),            # 12 px each, 8 shared: union 16
            det(rect(H, W, 8, 11, 0, 4), 0.8),           # 12 px inside the 16: 12 / 16
            det(rect(H, W, 14, 18, 8, 12), 0.7), det(rect(H, W, 18, 22, 12, 16), 0.7),
            det(rect(H, W, 0, 4, 10, 14), 0.6)]
    return tuple(dets), tuple(anns)
