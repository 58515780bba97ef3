"""Score the 6D DETECTION task — an unknown number of instances per image — and suppress duplicate poses: average precision of
pose estimates against ground truth under MSSD and MSPD, where every estimate counts and a false positive is punished (what
`evaluation.match_and_score`, the localization protocol, cannot say), for the chain depth_proposals -> label_proposals ->
infer_proposals -> verify / refine -> bop_csv_lines or any method that writes BOP results rows.

    ann = pose_annotations({scene: read_scene_gt(...)}, {scene: json.load(open(scene_gt_info.json))})
    res = score_pose_detections(read_bop_results(csv), ann, models, {scene: read_scene_camera(...)})     # {"AP", "AP_MSSD", "AP_MSPD", ...}
    keep = pose_nms(read_bop_results(csv), models)                                                       # rows without duplicate poses

The contract is "6D DETECTION SCORING" of include/picopose_hip.h (csrc/pp_pose_det.hip; tests/pose_detection_oracle.py restates it in
numpy loops).  It is the BOP 2024 6D-detection protocol WRITTEN FROM MEMORY: the BOP toolkit cannot be run next to this library, so
parity with it is UNPINNED.  What is exact: given the per-pair errors, the match tables and the kept rows equal the restatement bit
for bit.

The device computes the errors of all pairs (evaluation.pose_errors), the greedy matching per (group, metric, threshold)
(pp_pose_match) and the suppression walk per group (pp_pose_nms); grouping and sorting before, and the accumulation after, are
numpy on the host."""
import time

import numpy as np
import torch

from . import _lib
from . import scoring
from .evaluation import DEFAULT_WORKSPACE_BYTES, MSPD_THRESHOLDS, MSSD_THRESHOLDS, ObjectModels, _json, pose_errors

MAX_GROUP = _lib.PP_POSE_MAX_GROUP
MAX_METRICS = _lib.PP_POSE_MAX_METRICS
METRICS = ("mssd", "mspd")
REC_THRS = scoring.REC_THRS
MAX_PER_IMAGE = 100
_EST_KEYS = ("scene_id", "im_id", "obj_id", "score", "R", "t")


def read_image_targets(path):
    """test_targets_bop24.json (a path, or the decoded list of {"scene_id", "im_id"} rows) -> the sorted list of distinct
    (scene_id, im_id): what `images=` takes."""
    rows = _json(path)
    if not isinstance(rows, (list, tuple)):
        raise ValueError(f"image targets must be a list of rows, got {type(rows).__name__}")
    out = set()
    for i, r in enumerate(rows):
        if not isinstance(r, dict) or "scene_id" not in r or "im_id" not in r:
            raise ValueError(f"image target {i}: a row is {{'scene_id', 'im_id'}}, got {r!r}")
        out.add((int(r["scene_id"]), int(r["im_id"])))
    return sorted(out)


def _image_set(images):
    if images is None:
        return None
    try:
        return {(int(s), int(im)) for s, im in images}
    except (TypeError, ValueError):
        raise ValueError("images must be an iterable of (scene_id, im_id)") from None


def pose_annotations(ground_truth, gt_info=None, min_visib_fract=0.1):
    """The ground-truth side with its ignore flags.  ground_truth: {scene_id: evaluation.read_scene_gt(...)}; gt_info: None, or
    {scene_id: {im_id: [entries with "visib_fract"]}} — BOP's scene_gt_info.json content (its keys may be the file's strings) or what
    scene_gt.dataset_gt_info / format_gt_info produce — one entry per instance, in instance order.
    -> {"scene_id", "im_id", "obj_id", "inst" (N,) int64 (inst: the index within the image's scene_gt entry), "R" (N, 3, 3), "t" (N, 3)
    float64, "ignore" (N,) bool}, instances in (scene, image, instance) order of `ground_truth`.  ignore = visib_fract <
    min_visib_fract: BOP's rule AS REMEMBERED (an instance seen less than 10 % is neither required nor penalised; parity unpinned).
    Without gt_info nothing is ignored.  ValueError names the scene and image whose info is missing or of another length."""
    if not isinstance(ground_truth, dict):
        raise ValueError("ground_truth must be {scene_id: read_scene_gt(...)}")
    if not (isinstance(min_visib_fract, (int, float)) and min_visib_fract == min_visib_fract):
        raise ValueError(f"min_visib_fract must be a number, got {min_visib_fract!r}")
    cols = {k: [] for k in ("scene_id", "im_id", "obj_id", "inst", "ignore")}
    Rs, ts = [], []
    for s, per in ground_truth.items():
        info_s = None
        if gt_info is not None:
            info_s = gt_info.get(s, gt_info.get(int(s), gt_info.get(str(s))))
            if info_s is None:
                raise ValueError(f"gt_info holds no scene {s}")
        for im, gt in per.items():
            n = len(gt["obj_id"])
            ign = [False] * n
            if info_s is not None:
                info = info_s.get(im, info_s.get(int(im), info_s.get(str(im))))
                if info is None or len(info) != n:
                    raise ValueError(f"scene {s}, image {im}: {'no' if info is None else len(info)} info entries for {n} instances")
                for k, e in enumerate(info):
                    if not isinstance(e, dict) or "visib_fract" not in e:
                        raise ValueError(f"scene {s}, image {im}, instance {k}: no 'visib_fract'")
                ign = [bool(float(e["visib_fract"]) < min_visib_fract) for e in info]
            cols["scene_id"] += [int(s)] * n
            cols["im_id"] += [int(im)] * n
            cols["obj_id"] += [int(o) for o in np.asarray(gt["obj_id"]).tolist()]
            cols["inst"] += list(range(n))
            cols["ignore"] += ign
            Rs.append(np.asarray(gt["R"], dtype=np.float64).reshape(-1, 3, 3))
            ts.append(np.asarray(gt["t"], dtype=np.float64).reshape(-1, 3))
            if len(Rs[-1]) != n or len(ts[-1]) != n:
                raise ValueError(f"scene {s}, image {im}: {n} obj_ids for {len(Rs[-1])} rotations and {len(ts[-1])} translations")
    out = {k: np.array(v, dtype=bool if k == "ignore" else np.int64) for k, v in cols.items()}
    out["R"] = np.concatenate(Rs + [np.zeros((0, 3, 3))])
    out["t"] = np.concatenate(ts + [np.zeros((0, 3))])
    return out


def _estimate_columns(estimates, need_pose=True):
    """read_bop_results' dict, checked -> (keys [(scene, im)], obj (N,) int64, score (N,) float64); ValueError names the row."""
    if not isinstance(estimates, dict):
        raise ValueError("estimates must be evaluation.read_bop_results' dict")
    for k in _EST_KEYS if need_pose else _EST_KEYS[:4]:
        if k not in estimates:
            raise ValueError(f"estimates: no '{k}'")
    n = len(estimates["scene_id"])
    score = np.asarray(estimates["score"], dtype=np.float64).reshape(-1)
    obj = np.asarray(estimates["obj_id"]).reshape(-1)
    if len(estimates["im_id"]) != n or len(obj) != n or len(score) != n:
        raise ValueError(f"estimates: {n} scene_ids for {len(estimates['im_id'])} im_ids, {len(obj)} obj_ids and {len(score)} scores")
    if need_pose and (np.shape(estimates["R"]) != (n, 3, 3) or np.shape(estimates["t"]) != (n, 3)):
        raise ValueError(f"estimates: R must be ({n}, 3, 3) and t ({n}, 3), got {np.shape(estimates['R'])} and {np.shape(estimates['t'])}")
    bad = np.flatnonzero(~np.isfinite(score))
    if len(bad):
        raise ValueError(f"estimate {int(bad[0])}: 'score' must be a finite number, got {score[bad[0]]!r}")
    keys = list(zip(np.asarray(estimates["scene_id"]).astype(np.int64).tolist(), np.asarray(estimates["im_id"]).astype(np.int64).tolist()))
    return keys, obj.astype(np.int64), score


def _grouped_estimates(keys, obj, score, wanted, max_per_image):
    """-> {(image key, obj_id): rows by descending score, the lower row first among equals} after the images filter and the per-image cut."""
    per_image = {}
    for i, k in enumerate(keys):
        if wanted is None or k in wanted:
            per_image.setdefault(k, []).append(i)
    groups = {}
    for k, rows in per_image.items():
        rows = np.array(rows, np.int64)
        rows = rows[np.argsort(-score[rows], kind="stable")]                   # (rows ascend: stable = the lower row first)
        for i in rows[:max_per_image].tolist():
            groups.setdefault((k, int(obj[i])), []).append(i)
    return groups


def plan_groups(estimates, annotations, images=None, max_per_image=MAX_PER_IMAGE):
    """The groups, both axes and the pair blocks of 6D DETECTION SCORING, numpy arrays on the host.  estimates:
    evaluation.read_bop_results' dict; annotations: `pose_annotations`' dict; images: None, or an iterable of (scene_id, im_id) — the
    rows of a test_targets_bop24.json (`read_image_targets`): records of both sides outside it are dropped; max_per_image: the
    estimates kept per image, the best-scored first, the lower row first among equal scores (100: BOP's cap as remembered; None keeps all).
    -> {"images": the sorted (scene_id, im_id) keys that hold a record, "objects": the sorted obj_ids; one GROUP per (image, object)
    that holds a record, sorted by (image, object): "group_image", "group_object" (indices into the two lists), "group_est" and
    "group_gt" (n_groups, 2) = {first, count} on the estimate / ground-truth axis, "group_pair" the offset of the group's E_g x G_g
    estimate-major block; the ESTIMATE axis holds each group's kept estimates by descending score (the lower row first among equals):
    "est_index" (the row of `estimates`) and "est_score"; the GROUND-TRUTH axis holds each group's instances in annotation order:
    "gt_index" (the row of `annotations`) and "gt_ignore" uint8; "pair_est", "pair_gt" (n_pairs,): the estimates' and annotations'
    rows of every pair, in block order; "n_pairs"}.
    ValueError: a record column of the wrong length, a score that is not finite, a group with more than 4096 ground truths, 2^31 pairs."""
    if max_per_image is not None and not (isinstance(max_per_image, (int, np.integer)) and not isinstance(max_per_image, bool) and max_per_image > 0):
        raise ValueError(f"max_per_image must be None or a positive int, got {max_per_image!r}")
    keys, obj, score = _estimate_columns(estimates, need_pose=False)
    if not isinstance(annotations, dict) or any(k not in annotations for k in ("scene_id", "im_id", "obj_id", "ignore")):
        raise ValueError("annotations must be pose_annotations' dict")
    wanted = _image_set(images)
    est_groups = _grouped_estimates(keys, obj, score, wanted, max_per_image)
    gt_groups = {}
    gkeys = zip(np.asarray(annotations["scene_id"]).tolist(), np.asarray(annotations["im_id"]).tolist(), np.asarray(annotations["obj_id"]).tolist())
    for i, (s, im, o) in enumerate(gkeys):
        if wanted is None or (s, im) in wanted:
            gt_groups.setdefault(((s, im), int(o)), []).append(i)
    gkeys = sorted(set(est_groups) | set(gt_groups))
    img_list = sorted({k[0] for k in gkeys})
    obj_list = sorted({k[1] for k in gkeys})
    img_of, obj_of = {k: i for i, k in enumerate(img_list)}, {o: i for i, o in enumerate(obj_list)}
    est_lists = [np.array(est_groups.get(k, []), np.int64) for k in gkeys]
    gt_lists = [np.array(gt_groups.get(k, []), np.int64) for k in gkeys]
    group_est, group_gt, group_pair, est_index, gt_index, n_pairs = scoring.plan_groups(gkeys, est_lists, gt_lists, MAX_GROUP, "object",
                                                                                        "ground truths")
    scoring.check_offsets(n_pairs, "call", max(len(est_index), len(gt_index)))
    pair_est = np.concatenate([np.repeat(e, len(g)) for e, g in zip(est_lists, gt_lists)] + [np.zeros(0, np.int64)])
    pair_gt = np.concatenate([np.tile(g, len(e)) for e, g in zip(est_lists, gt_lists)] + [np.zeros(0, np.int64)])
    return {"images": img_list, "objects": obj_list, "group_image": np.array([img_of[k[0]] for k in gkeys], np.int64),
            "group_object": np.array([obj_of[k[1]] for k in gkeys], np.int64), "group_est": group_est, "group_gt": group_gt,
            "group_pair": group_pair, "est_index": est_index, "est_score": score[est_index], "gt_index": gt_index,
            "gt_ignore": np.asarray(annotations["ignore"]).astype(np.uint8)[gt_index], "pair_est": pair_est, "pair_gt": pair_gt,
            "n_pairs": n_pairs}


def match_pose_errors(plan, errors, limits, device="cuda", timings=None):
    """The kernel-level call: pp_pose_match on `plan_groups`' plan with the caller's errors.  errors: (M, n_pairs) float32, a numpy
    array or a tensor (on `device`, or uploaded), row m the errors of metric m in the plan's block order; limits (n_groups, M, T)
    float64: what an error must stay below.  1 <= M <= 4, T >= 1.
    -> {"est_match" (M, T, n_est) int32: the position on the ground-truth axis of the matched instance or -1, "est_ignore" (M, T,
    n_est) uint8, "gt_match" (M, T, n_gt) int32: the position on the estimate axis or -1} as numpy.  A plan without groups gives empty
    tables without touching the device.  timings: a dict that receives the device seconds of the launch under "match".
    ValueError: a shape or dtype mismatch, M outside 1 .. 4, a NaN limit."""
    n_groups, n_pairs = len(plan["group_pair"]), int(plan["n_pairs"])
    n_est, n_gt = len(plan["est_index"]), len(plan["gt_index"])
    lim = np.ascontiguousarray(limits, dtype=np.float64)
    if lim.ndim != 3 or lim.shape[0] != n_groups or lim.shape[2] == 0:
        raise ValueError(f"limits must be (n_groups = {n_groups}, M, T >= 1), got {lim.shape}")
    M, T = lim.shape[1], lim.shape[2]
    if not 1 <= M <= MAX_METRICS:
        raise ValueError(f"limits: M must be 1 .. {MAX_METRICS}, got {M}")
    if np.isnan(lim).any():
        g, m, t = (int(v[0]) for v in np.nonzero(np.isnan(lim)))
        raise ValueError(f"limits[{g}, {m}, {t}] is NaN")
    is_tensor = isinstance(errors, torch.Tensor)
    if tuple(errors.shape) != (M, n_pairs) or errors.dtype != (torch.float32 if is_tensor else np.float32):
        raise ValueError(f"errors must be (M = {M}, n_pairs = {n_pairs}) float32, got {errors.dtype} {tuple(errors.shape)}")
    if int(plan["group_gt"][:, 1].max(initial=0)) > MAX_GROUP:
        raise ValueError(f"a group holds more than {MAX_GROUP} ground truths")
    out = {"est_match": np.full((M, T, n_est), -1, np.int32), "est_ignore": np.zeros((M, T, n_est), np.uint8),
           "gt_match": np.full((M, T, n_gt), -1, np.int32)}
    if n_groups == 0:
        return out
    dev = scoring.require_cuda(device, "match_pose_errors")
    up = scoring.uploader(dev)
    groups = scoring.group_rows(plan["group_est"], plan["group_gt"], plan["group_pair"])
    err_d = (errors.to(dev) if is_tensor else up(errors)).contiguous()
    if n_pairs == 0:
        err_d = torch.zeros(1, dtype=torch.float32, device=dev)
    groups_d, lim_d, ign_d = up(groups.ravel()), up(lim.ravel()), up(plan["gt_ignore"], side=True)
    em = torch.full((M, T, max(n_est, 1)), -1, dtype=torch.int32, device=dev)
    ei = torch.zeros((M, T, max(n_est, 1)), dtype=torch.uint8, device=dev)
    gm = torch.full((M, T, max(n_gt, 1)), -1, dtype=torch.int32, device=dev)
    mark, finish = scoring.device_marks(timings)
    mark("match")
    _lib.call("pp_pose_match", err_d, M, n_pairs, groups_d, groups, n_groups, n_est, n_gt, ign_d, lim_d, lim, T, em, ei, gm)
    mark("match")
    out["est_match"], out["est_ignore"], out["gt_match"] = em.cpu().numpy()[:, :, :n_est], ei.cpu().numpy()[:, :, :n_est], gm.cpu().numpy()[:, :, :n_gt]
    finish()
    return out


def _thresholds(name, v):
    a = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    if a.size == 0 or not np.all(np.isfinite(a)) or np.any(a <= 0):
        raise ValueError(f"{name} must be a non-empty list of positive numbers, got {v!r}")
    return a


def _check_objects(models, obj_ids, rows, what):
    """Every kept row's obj_id must be known to the models; ValueError names the row."""
    if not isinstance(models, ObjectModels):
        raise ValueError("models must be an evaluation.ObjectModels")
    for i in np.sort(rows).tolist():
        if int(obj_ids[i]) not in models.index:
            raise ValueError(f"{what} {i}: unknown obj_id {int(obj_ids[i])}: the models hold {models.obj_ids}")


def match_poses(estimates, annotations, models, cameras, image_width=640, thresholds_mssd=MSSD_THRESHOLDS, thresholds_mspd=MSPD_THRESHOLDS,
                images=None, max_per_image=MAX_PER_IMAGE, workspace_bytes=DEFAULT_WORKSPACE_BYTES, timings=None):
    """Estimates against ground truth -> the match tables of 6D DETECTION SCORING and everything `accumulate` needs: `plan_groups`'
    plan, `match_pose_errors`' tables, "metrics" = ("mssd", "mspd"), "thresholds" (2, T), "limits" (n_groups, 2, T) float64 and
    "errors" (2, n_pairs) float32 numpy (MSSD, MSPD in the plan's block order).
    models: evaluation.ObjectModels; cameras: {scene_id: read_scene_camera(...)}.  The errors of ALL pairs of all groups come from one
    evaluation.pose_errors call (which chunks itself under `workspace_bytes`).  An estimate is correct at a threshold when its error is
    below the limit: MSSD threshold x the object's diameter; MSPD threshold x image_width / 640 pixels — both lists must have one
    length.  timings: a dict that receives the device seconds of the "errors" and "match" launches and "total", the wall-clock
    seconds of the call.  ValueError before any device work: what `plan_groups` raises, an obj_id unknown to `models`, an image with
    pairs but no camera, threshold lists of different lengths."""
    t_start = time.perf_counter()
    th_s, th_p = _thresholds("thresholds_mssd", thresholds_mssd), _thresholds("thresholds_mspd", thresholds_mspd)
    if len(th_s) != len(th_p):
        raise ValueError(f"thresholds_mssd and thresholds_mspd must have one length, got {len(th_s)} and {len(th_p)}")
    th = np.stack([th_s, th_p])
    if not (isinstance(image_width, (int, float)) and image_width > 0):
        raise ValueError(f"image_width must be a positive number, got {image_width!r}")
    plan = plan_groups(estimates, annotations, images, max_per_image)
    _estimate_columns(estimates)
    _check_objects(models, np.asarray(estimates["obj_id"]), plan["est_index"], "estimate")
    _check_objects(models, np.asarray(annotations["obj_id"]), plan["gt_index"], "annotation")
    pe, pg, n = plan["pair_est"], plan["pair_gt"], plan["n_pairs"]
    K = np.zeros((n, 3, 3))
    cam_of = {}
    for i, (s, im) in enumerate(zip(np.asarray(annotations["scene_id"])[pg].tolist(), np.asarray(annotations["im_id"])[pg].tolist())):
        if (s, im) not in cam_of:
            if s not in cameras or im not in cameras[s]:
                raise ValueError(f"cameras holds no entry for scene {s}, image {im}, which has estimates to score")
            cam_of[(s, im)] = np.asarray(cameras[s][im]["K"], dtype=np.float64).reshape(3, 3)
        K[i] = cam_of[(s, im)]
    diam = np.array([models.diameter(plan["objects"][o]) for o in plan["group_object"]], dtype=np.float64)
    limits = np.stack([diam[:, None] * th[0][None], np.broadcast_to(th[1][None] * (float(image_width) / 640.0), (len(diam), th.shape[1]))], axis=1)
    mark, finish = scoring.device_marks(timings if n else None)
    mark("errors")
    err = pose_errors(models, np.asarray(estimates["obj_id"])[pe], np.asarray(estimates["R"], dtype=np.float64)[pe],
                      np.asarray(estimates["t"], dtype=np.float64)[pe], np.asarray(annotations["R"])[pg], np.asarray(annotations["t"])[pg],
                      K=K, kinds=METRICS, workspace_bytes=workspace_bytes)
    mark("errors")
    errors = torch.stack([err["mssd"], err["mspd"]])
    out = dict(plan, metrics=METRICS, thresholds=th, limits=limits)
    out.update(match_pose_errors(plan, errors, limits.reshape(len(diam), 2, -1), device=models.device, timings=timings))
    out["errors"] = errors.cpu().numpy()
    finish()
    if timings is not None:
        timings["total"] = timings.get("total", 0.0) + time.perf_counter() - t_start
    return out


def accumulate(matches):
    """match_poses' result (or a plan plus `match_pose_errors`' tables) -> {"precision" (M, T, 101, K), "recall" (M, T, K)} float64, K the
    objects, plus "objects" and "metrics": per object, metric and threshold the estimates of all images, sorted by descending score
    (mergesort), through `scoring.pr_curve` (recall: 0 without estimates).  An object without a non-ignored ground truth stays -1."""
    m = matches
    M, T = m["est_match"].shape[:2]
    objects = m["objects"]
    precision, recall = -np.ones((M, T, 101, len(objects))), -np.ones((M, T, len(objects)))
    span = lambda rows: np.concatenate([np.arange(s, s + n) for s, n in rows] + [np.zeros(0, np.int64)]).astype(np.int64)   # noqa: E731
    for k in range(len(objects)):
        rows = np.nonzero(m["group_object"] == k)[0]
        npig = int(np.count_nonzero(m["gt_ignore"][span(m["group_gt"][rows])] == 0))
        if npig == 0:
            continue
        sel = span(m["group_est"][rows])
        sel = sel[np.argsort(-m["est_score"][sel], kind="mergesort")]
        for mi in range(M):
            precision[mi, :, :, k], recall[mi, :, k] = scoring.pr_curve(m["est_match"][mi][:, sel] >= 0, m["est_ignore"][mi][:, sel] != 0, npig)
    return {"precision": precision, "recall": recall, "objects": objects, "metrics": tuple(m.get("metrics", METRICS[:M]))}


def summarize(acc):
    """accumulate's result -> {"AP_MSSD", "AP_MSPD": the mean over the objects that have a non-ignored ground truth of the mean over
    thresholds and recall samples (-1 when there is no such object), "AP" = (AP_MSSD + AP_MSPD) / 2, "per_object": {obj_id: {"AP_MSSD",
    "AP_MSPD", "AP"}} (-1 for an object that does not count), "recall": {metric: (T, K) the recall at the last estimate}, "objects"}.  The
    names follow acc["metrics"]."""
    p, names = acc["precision"], [f"AP_{n.upper()}" for n in acc["metrics"]]
    K = p.shape[3]
    cell = np.array([[float(np.mean(p[mi, :, :, k])) if p.shape[1] and np.all(p[mi, :, :, k] > -1) else -1.0 for k in range(K)]
                     for mi in range(len(names))]).reshape(len(names), K)
    both = lambda v: float(np.mean(v)) if all(x > -1 for x in v) else -1.0      # noqa: E731
    out = {n: scoring.mean_valid(cell[mi]) for mi, n in enumerate(names)}
    out["AP"] = both([out[n] for n in names])
    out["per_object"] = {o: dict({n: float(cell[mi, k]) for mi, n in enumerate(names)}, AP=both(cell[:, k].tolist()))
                         for k, o in enumerate(acc["objects"])}
    out["recall"] = {n: acc["recall"][mi] for mi, n in enumerate(acc["metrics"])}
    out["objects"] = list(acc["objects"])
    return out


def score_pose_detections(estimates, annotations, models, cameras, **kw):
    """summarize(accumulate(match_poses(estimates, annotations, models, cameras, **kw))): AP, AP_MSSD, AP_MSPD, per_object and the recalls
    in one call."""
    return summarize(accumulate(match_poses(estimates, annotations, models, cameras, **kw)))


def plan_nms(estimates, images=None):
    """Host side of `pose_nms`: the groups (image, obj_id) sorted by (image, object), each group's rows by descending score (the lower
    row first among equals; no per-image cut), and the triangle of pairs -> {"group_est" (n_groups, 2) {first, count}, "group_tri" the
    triangle offsets, "group_obj" the obj_ids, "est_index" (n_est,), "tri_early", "tri_late" (n_tri,): the rows of the earlier i and the
    later j of every pair, at offset + j (j - 1) / 2 + i, "n_tri"}.  ValueError: a group above 4096 estimates, 2^31 pairs."""
    keys, obj, score = _estimate_columns(estimates)
    groups = _grouped_estimates(keys, obj, score, _image_set(images), None)
    gkeys = sorted(groups)
    lists = [np.array(groups[k], np.int64) for k in gkeys]
    group_est, est_index = scoring.axis(gkeys, lists, MAX_GROUP, "object", "estimates")
    tri = group_est[:, 1] * (group_est[:, 1] - 1) // 2
    if int(tri.sum()) >= 2 ** 31:
        raise ValueError(f"{int(tri.sum())} pairs in one call: more than 32-bit offsets hold")
    early, late = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for e in lists:
        j, i = np.tril_indices(len(e), -1)                                     # row-major over j, i < j: offset j (j - 1) / 2 + i
        early.append(e[i])
        late.append(e[j])
    return {"group_est": group_est, "group_tri": scoring.first(tri), "group_obj": np.array([k[1] for k in gkeys], np.int64),
            "est_index": est_index, "tri_early": np.concatenate(early), "tri_late": np.concatenate(late),
            "n_tri": int(tri.sum())}


def nms_walk(plan, dist, limit, device="cuda", timings=None):
    """The kernel-level call: pp_pose_nms on `plan_nms`' plan with the caller's distances.  dist (n_tri,) float32 numpy or tensor, limit
    (n_groups,) float64, not negative -> keep (n_est,) uint8 numpy on the plan's estimate axis.  ValueError: a shape or dtype mismatch, a
    limit that is NaN or negative."""
    n_groups, n_est, n_tri = len(plan["group_tri"]), len(plan["est_index"]), int(plan["n_tri"])
    lim = np.ascontiguousarray(limit, dtype=np.float64)
    if lim.shape != (n_groups,) or not np.all(lim >= 0):
        raise ValueError(f"limit must be (n_groups = {n_groups},) float64 and not negative, got {lim.shape} {lim[~(lim >= 0)][:1] if lim.shape == (n_groups,) else ''}")
    is_tensor = isinstance(dist, torch.Tensor)
    if tuple(dist.shape) != (n_tri,) or dist.dtype != (torch.float32 if is_tensor else np.float32):
        raise ValueError(f"dist must be (n_tri = {n_tri},) float32, got {dist.dtype} {tuple(dist.shape)}")
    if n_groups == 0:
        return np.zeros(0, np.uint8)
    dev = scoring.require_cuda(device, "nms_walk")
    up = scoring.uploader(dev)
    groups = np.ascontiguousarray(np.concatenate([plan["group_est"], plan["group_tri"][:, None]], axis=1), dtype=np.int32)
    dist_d = (dist.to(dev) if is_tensor else up(dist)).contiguous() if n_tri else torch.zeros(1, dtype=torch.float32, device=dev)
    groups_d, lim_d = up(groups.ravel()), up(lim)
    keep = torch.zeros(n_est, dtype=torch.uint8, device=dev)
    mark, finish = scoring.device_marks(timings)
    mark("nms")
    _lib.call("pp_pose_nms", dist_d, n_tri, groups_d, groups, n_groups, n_est, lim_d, lim, keep)
    mark("nms")
    out = keep.cpu().numpy()
    finish()
    return out


def pose_nms(estimates, models, nms_dist=0.1, images=None, device="cuda", timings=None):
    """Suppress duplicate poses: the rows of `estimates` (read_bop_results' dict) that survive, ascending (input order).  Per (image,
    obj_id) the estimates are visited by descending score (the lower row first among equals); one is dropped when an earlier KEPT
    estimate i of the group lies within nms_dist x the object's diameter of it, the distance being the MSSD with i as the ground truth
    and the later one as the estimate (pose_errors(R_est=R_j, R_gt=R_i), the symmetries of `models` included; only this triangle is
    computed).  A dropped estimate suppresses nothing; a distance exactly at the limit keeps.  images: as `plan_groups` takes them — rows
    outside are not returned.  This is the project's own rule: nms_dist = 0.1 is NOT tuned, and its effect on real data is unmeasured.
    timings: a dict that receives the device seconds under "nms_errors" and "nms".  ValueError before any device work: a row with
    an obj_id unknown to `models`, a score that is not finite, a group above 4096 estimates, nms_dist negative or not finite."""
    if not (isinstance(nms_dist, (int, float)) and 0 <= nms_dist < float("inf")):
        raise ValueError(f"nms_dist must be a finite number >= 0, got {nms_dist!r}")
    plan = plan_nms(estimates, images)
    _check_objects(models, np.asarray(estimates["obj_id"]), plan["est_index"], "estimate")
    if len(plan["est_index"]) == 0:
        return np.zeros(0, np.int64)
    R, t = np.asarray(estimates["R"], dtype=np.float64), np.asarray(estimates["t"], dtype=np.float64)
    i, j = plan["tri_early"], plan["tri_late"]
    mark, finish = scoring.device_marks(timings if len(i) else None)
    mark("nms_errors")
    dist = pose_errors(models, np.asarray(estimates["obj_id"])[j], R[j], t[j], R[i], t[i], kinds=("mssd",))["mssd"]
    mark("nms_errors")
    finish()
    limit = float(nms_dist) * np.array([models.diameter(o) for o in plan["group_obj"]], dtype=np.float64)
    keep = nms_walk(plan, dist, limit, device=device, timings=timings)
    return np.sort(plan["est_index"][keep != 0])
