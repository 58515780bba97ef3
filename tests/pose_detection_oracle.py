"""numpy restatement of 6D DETECTION SCORING (include/picopose_hip.h) in literal loops: grouping, the per-image cut and the ordering,
the greedy matching as the SCAN over the estimates in order, the duplicate-pose walk, the accumulation and the summary.  The matcher
and the walk take the ERROR ARRAYS as inputs (the pose errors themselves are held by test_evaluation_gpu.py), so the device tables
are compared bit for bit: nothing here or there accumulates in floating point before the accumulation.  Nothing is imported from
the package."""
import numpy as np

MAX_GROUP = 4096
REC_THRS = np.linspace(0, 1, 101)
TABLES = ("est_match", "est_ignore", "gt_match")
LAYOUT = ("group_image", "group_object", "group_est", "group_gt", "group_pair", "est_index", "est_score", "gt_index", "gt_ignore",
          "pair_est", "pair_gt")


def annotations(ground_truth, gt_info=None, min_visib_fract=0.1):
    """{scene: {im: {"obj_id", "R", "t"}}} (and {scene: {im: [{"visib_fract"}]}}) -> the flat ground-truth side with ignore flags."""
    out = {k: [] for k in ("scene_id", "im_id", "obj_id", "inst", "ignore", "R", "t")}
    for s, per in ground_truth.items():
        for im, gt in per.items():
            for k in range(len(gt["obj_id"])):
                out["scene_id"].append(int(s))
                out["im_id"].append(int(im))
                out["obj_id"].append(int(gt["obj_id"][k]))
                out["inst"].append(k)
                out["ignore"].append(False if gt_info is None else bool(gt_info[s][im][k]["visib_fract"] < min_visib_fract))
                out["R"].append(np.asarray(gt["R"][k], np.float64))
                out["t"].append(np.asarray(gt["t"][k], np.float64))
    res = {k: np.array(out[k], dtype=bool if k == "ignore" else np.int64) for k in ("scene_id", "im_id", "obj_id", "inst", "ignore")}
    res["R"] = np.array(out["R"], np.float64).reshape(-1, 3, 3)
    res["t"] = np.array(out["t"], np.float64).reshape(-1, 3)
    return res


def _kept_estimates(estimates, wanted, max_per_image):
    """-> {(image, obj): rows in group order}: per image the max_per_image best (score descending, then row), then per object."""
    per_image = {}
    for i in range(len(estimates["score"])):
        key = (int(estimates["scene_id"][i]), int(estimates["im_id"][i]))
        if wanted is None or key in wanted:
            per_image.setdefault(key, []).append(i)
    groups = {}
    for key, rows in per_image.items():
        rows = sorted(rows, key=lambda i: (-float(estimates["score"][i]), i))
        if max_per_image is not None:
            rows = rows[:max_per_image]
        for i in rows:                                                          # (already by descending score, then row)
            groups.setdefault((key, int(estimates["obj_id"][i])), []).append(i)
    return groups


def plan(estimates, ann, images=None, max_per_image=100):
    wanted = None if images is None else {(int(s), int(im)) for s, im in images}
    est_groups = _kept_estimates(estimates, wanted, max_per_image)
    gt_groups = {}
    for i in range(len(ann["obj_id"])):
        key = (int(ann["scene_id"][i]), int(ann["im_id"][i]))
        if wanted is None or key in wanted:
            gt_groups.setdefault((key, int(ann["obj_id"][i])), []).append(i)
    keys = sorted(set(est_groups) | set(gt_groups))
    image_list, object_list = sorted({k[0] for k in keys}), sorted({k[1] for k in keys})
    out = {k: [] for k in LAYOUT}
    e0 = g0 = p0 = 0
    for k in keys:
        est, gts = est_groups.get(k, []), gt_groups.get(k, [])
        out["group_image"].append(image_list.index(k[0]))
        out["group_object"].append(object_list.index(k[1]))
        out["group_est"].append([e0, len(est)])
        out["group_gt"].append([g0, len(gts)])
        out["group_pair"].append(p0)
        out["est_index"] += est
        out["est_score"] += [float(estimates["score"][i]) for i in est]
        out["gt_index"] += gts
        out["gt_ignore"] += [int(ann["ignore"][i]) for i in gts]
        for e in est:
            for g in gts:
                out["pair_est"].append(e)
                out["pair_gt"].append(g)
        e0, g0, p0 = e0 + len(est), g0 + len(gts), p0 + len(est) * len(gts)
    dt = {"est_score": np.float64, "gt_ignore": np.uint8}
    res = {k: np.array(v, dtype=dt.get(k, np.int64)) for k, v in out.items()}
    res["group_est"], res["group_gt"] = res["group_est"].reshape(-1, 2), res["group_gt"].reshape(-1, 2)
    res.update(images=image_list, objects=object_list, n_pairs=p0)
    return res


def match(pl, errors, limits):
    """The scan.  errors (M, n_pairs) float32, limits (n_groups, M, T) float64 -> est_match, est_ignore, gt_match."""
    errors, limits = np.asarray(errors), np.asarray(limits, np.float64)
    assert errors.dtype == np.float32
    M, T = limits.shape[1], limits.shape[2]
    n_est, n_gt = len(pl["est_index"]), len(pl["gt_index"])
    est_match, est_ignore = np.full((M, T, n_est), -1, np.int32), np.zeros((M, T, n_est), np.uint8)
    gt_match = np.full((M, T, n_gt), -1, np.int32)
    for g in range(len(pl["group_pair"])):
        (e0, ne), (g0, ng), off = pl["group_est"][g], pl["group_gt"][g], int(pl["group_pair"][g])
        for m in range(M):
            for t in range(T):
                lim = float(limits[g, m, t])
                matched = [False] * ng
                for e in range(ne):
                    winner = {False: -1, True: -1}                               # per class: not ignored, ignored
                    for j in range(ng):
                        v = errors[m, off + e * ng + j]
                        if matched[j] or np.signbit(v) or not float(v) < lim:    # (a NaN and +inf fail the comparison)
                            continue
                        ig = bool(pl["gt_ignore"][g0 + j])
                        w = winner[ig]
                        if w < 0 or v < errors[m, off + e * ng + w]:             # strict: the lowest index among equals stays
                            winner[ig] = j
                    w, ig = (winner[False], False) if winner[False] >= 0 else (winner[True], True)
                    if w >= 0:
                        matched[w] = True
                        est_match[m, t, e0 + e], est_ignore[m, t, e0 + e], gt_match[m, t, g0 + w] = g0 + w, ig, e0 + e
    return {"est_match": est_match, "est_ignore": est_ignore, "gt_match": gt_match}


def plan_nms(estimates, images=None):
    wanted = None if images is None else {(int(s), int(im)) for s, im in images}
    groups = _kept_estimates(estimates, wanted, None)
    out = {"group_est": [], "group_tri": [], "group_obj": [], "est_index": [], "tri_early": [], "tri_late": []}
    e0 = t0 = 0
    for k in sorted(groups):
        est = groups[k]
        out["group_est"].append([e0, len(est)])
        out["group_tri"].append(t0)
        out["group_obj"].append(k[1])
        out["est_index"] += est
        for j in range(len(est)):
            for i in range(j):
                out["tri_early"].append(est[i])
                out["tri_late"].append(est[j])
        e0, t0 = e0 + len(est), t0 + len(est) * (len(est) - 1) // 2
    res = {k: np.array(v, np.int64) for k, v in out.items()}
    res["group_est"] = res["group_est"].reshape(-1, 2)
    res["n_tri"] = t0
    return res


def nms(pl, dist, limit):
    """The walk.  dist (n_tri,) float32, limit (n_groups,) float64 -> keep (n_est,) uint8."""
    dist = np.asarray(dist)
    assert dist.dtype == np.float32
    keep = np.zeros(len(pl["est_index"]), np.uint8)
    for g in range(len(pl["group_tri"])):
        (e0, ne), off = pl["group_est"][g], int(pl["group_tri"][g])
        for j in range(ne):
            dropped = False
            for i in range(j):
                if keep[e0 + i] and float(dist[off + j * (j - 1) // 2 + i]) < float(limit[g]):
                    dropped = True
            keep[e0 + j] = not dropped
    return keep


def accumulate(m):
    M, T = m["est_match"].shape[:2]
    K = len(m["objects"])
    precision, recall = -np.ones((M, T, 101, K)), -np.ones((M, T, K))
    for k in range(K):
        est, npig = [], 0
        for g in range(len(m["group_pair"])):
            if m["group_object"][g] != k:
                continue
            est += list(range(m["group_est"][g][0], m["group_est"][g][0] + m["group_est"][g][1]))
            for j in range(m["group_gt"][g][0], m["group_gt"][g][0] + m["group_gt"][g][1]):
                npig += int(m["gt_ignore"][j] == 0)
        if npig == 0:
            continue
        est = np.array(est, np.int64)
        est = est[np.argsort(-m["est_score"][est], kind="mergesort")]
        for mi in range(M):
            for t in range(T):
                tp = fp = 0
                rc, pr = np.zeros(len(est)), np.zeros(len(est))
                for n, e in enumerate(est):
                    if not m["est_ignore"][mi, t, e]:
                        if m["est_match"][mi, t, e] >= 0:
                            tp += 1
                        else:
                            fp += 1
                    rc[n] = float(tp) / npig
                    pr[n] = float(tp) / (float(fp) + float(tp) + np.spacing(1))
                for n in range(len(est) - 2, -1, -1):
                    pr[n] = max(pr[n], pr[n + 1])
                recall[mi, t, k] = rc[-1] if len(est) else 0
                ind = np.searchsorted(rc, REC_THRS, side="left")
                for r in range(101):
                    precision[mi, t, r, k] = pr[ind[r]] if ind[r] < len(est) else 0.0
    return {"precision": precision, "recall": recall, "objects": m["objects"], "metrics": tuple(m.get("metrics", ("mssd", "mspd")[:M]))}


def summarize(acc):
    p = acc["precision"]
    out, per = {}, {o: {} for o in acc["objects"]}
    for mi, name in enumerate(acc["metrics"]):
        cells = []
        for k, o in enumerate(acc["objects"]):
            c = float(np.mean(p[mi, :, :, k])) if np.all(p[mi, :, :, k] > -1) else -1.0
            per[o]["AP_" + name.upper()] = c
            if c > -1:
                cells.append(c)
        out["AP_" + name.upper()] = float(np.mean(cells)) if cells else -1.0
    names = ["AP_" + n.upper() for n in acc["metrics"]]
    out["AP"] = float(np.mean([out[n] for n in names])) if all(out[n] > -1 for n in names) else -1.0
    for o in per:
        per[o]["AP"] = float(np.mean([per[o][n] for n in names])) if all(per[o][n] > -1 for n in names) else -1.0
    out["per_object"] = per
    return out


def score(pl, errors, limits, metrics=("mssd", "mspd")):
    """summarize(accumulate(...)) of the plan, the errors and the limits."""
    return summarize(accumulate(dict(pl, metrics=metrics, **match(pl, errors, limits))))
