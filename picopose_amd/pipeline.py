"""Per-batch inference as the reference's evaluator runs it (run_test.py:151-186): network forward, then
PnP/RANSAC for every (instance, hypothesis), hypotheses ranked by inlier ratio, stage-2 pose as the
fallback when PnP fails.  One batched PnP launch and one device->host copy per batch instead of the
reference's B*hyp host round trips.

on_saturation: what a mini-batch whose forward clamped an f16x3 / f16 operand (ops.saturation_word) turns into.  "raise" (default): the
PicoPoseHipError of pose_recovery.py.  "exact": a snapshot of the word is taken on the forward's stream right after it
(ops.saturation_take), travels with the batch's poses, and a set snapshot re-runs that mini-batch alone in strict fp32 (Net.precision = "f32",
match_mode = "exact") — its poses are then the f32 network's, the other mini-batches keep the fast mode's; net.range_fallbacks counts the
re-runs.  The snapshot is taken from the word of the batch's own device, so several devices keep separate verdicts (by construction: the
tests have one GPU).

pnp_refine: None (default) | "lm" — the batched PnP refines each pose by Levenberg-Marquardt on its RANSAC consensus set
(utils/pose_recovery.py, refine="lm").  Only R and t move: the inlier ratios, the success flags and therefore the order of the
hypotheses are those of pnp_refine=None.

depth / depth_scale / depth_unit / rgbd_inlier_dist: with the test depth image every hypothesis also carries the pose of the batched
3D-3D RANSAC (rgbd_pose.py, pp_rgbd_ransac) on the same correspondences: 'R_rgbd', 't_rgbd', 'rgbd_inliers_ratio', 'rgbd_success'.
The PnP results, the ranking and the order of the hypotheses are those of a call without depth."""
import numpy as np
import torch

from . import ops
from .utils.pose_recovery import check_refine, pose_recovery_ransac_pnp_batched

ON_SATURATION = ("raise", "exact")


def pnp_inputs(outputs, real_K):
    """The (hyp*B) PnP problems of a forward, hypothesis-major: arguments of pose_recovery_ransac_pnp_batched."""
    hyp = len(outputs)
    cat = lambda k: torch.cat([o[k] for o in outputs], dim=0)  # noqa: E731
    return (cat("tar_pts_2d"), cat("src_pts_3d"), real_K.repeat(hyp, 1, 1), cat("tem_pose"), cat("pred_tar_pts"),
            cat("pred_src_pts"))


def pnp_for_outputs(outputs, real_K, return_npts=False, sat_slot=None, pnp_refine=None):
    """outputs: list (hyp) of Net.forward dicts; real_K (B,3,3) -> rot (hyp,B,3,3), tvec (hyp,B,3,1), ratio, ok
    [+ npts (hyp,B): correspondences each problem received] [+ saturated (bool): the forward's snapshot `sat_slot` was set].
    pnp_refine="lm": rot / tvec are the refined poses (module docstring); ratio, ok and npts are pnp_refine=None's."""
    hyp, B = len(outputs), outputs[0]["pred_poses"].shape[0]
    res = pose_recovery_ransac_pnp_batched(*pnp_inputs(outputs, real_K), return_npts=return_npts, sat_slot=sat_slot, refine=pnp_refine)
    rot, tvec, ratio, ok = res[:4]
    out = (rot.reshape(hyp, B, 3, 3), tvec.reshape(hyp, B, 3, 1), ratio.reshape(hyp, B), ok.reshape(hyp, B))
    out = out + (res[4].reshape(hyp, B),) if return_npts else out
    return out + (res[-1],) if sat_slot is not None else out


def pnp_for_outputs_async(outputs, real_K, host=None, stream=None, sat_slot=None, pnp_refine=None):
    """pnp_for_outputs without the host wait -> handle; `pnp_collect(handle, hyp, B)` reads it (one batch later in a serving loop).
    stream: run the PnP launch and the copy on this side stream, beside the next batch's forward (pose_recovery_ransac_pnp_batched_async).
    sat_slot: the forward's saturation snapshot rides in the copy; `handle.saturated` holds it after pnp_collect.
    pnp_refine: as pnp_for_outputs."""
    from .utils.pose_recovery import pose_recovery_ransac_pnp_batched_async

    return pose_recovery_ransac_pnp_batched_async(*pnp_inputs(outputs, real_K), host=host, stream=stream, sat_slot=sat_slot,
                                                  refine=pnp_refine)


def pnp_collect(handle, hyp, B):
    rot, tvec, ratio, ok = handle.result()[:4]     # (a refining launch appends its refine_stats)
    return rot.reshape(hyp, B, 3, 3), tvec.reshape(hyp, B, 3, 1), ratio.reshape(hyp, B), ok.reshape(hyp, B)


def _rgbd_args(outputs, real_K, inlier_dist, image_index):
    """inlier_dist / image_index per instance (B,) (or a number / None) -> per problem (hyp * B,), hypothesis-major like pnp_inputs."""
    hyp, B = len(outputs), outputs[0]["pred_poses"].shape[0]
    per_problem = lambda x: x if x is None or np.ndim(x) == 0 or tuple(np.shape(x)) != (B,) else (  # noqa: E731
        x.repeat(hyp) if isinstance(x, torch.Tensor) else np.tile(np.asarray(x), hyp))
    return hyp, B, per_problem(inlier_dist), per_problem(image_index)


def _rgbd_shaped(res, hyp, B):
    rot, tvec, ratio, ok, npts, st = res[:6]
    out = (rot.reshape(hyp, B, 3, 3), tvec.reshape(hyp, B, 3, 1), ratio.reshape(hyp, B), ok.reshape(hyp, B), npts.reshape(hyp, B),
           {k: v.reshape(hyp, B) for k, v in st.items()})
    return out + (res[6].reshape(hyp, B, -1),) if len(res) > 6 else out


def rgbd_for_outputs(outputs, real_K, depth, inlier_dist, image_index=None, **kw):
    """The RGB-D pose of every (hypothesis, instance) of a forward (rgbd_pose.pose_recovery_ransac_rgbd_batched over pnp_inputs):
    outputs: list (hyp) of Net.forward dicts; real_K (B,3,3); depth (dH, dW) or (n_images, dH, dW); inlier_dist a number or one per
    instance (B,) (or per problem (hyp * B,)), in the unit of the network's 3-D points; image_index (B,) (or (hyp * B,)): the depth
    image of each instance (default 0); **kw: iterations, return_inliers, depth_scale, depth_unit.
    -> rot (hyp,B,3,3), tvec (hyp,B,3,1), ratio, ok, npts (hyp,B), stats dict of (hyp,B) arrays [+ inliers (hyp,B,N)]."""
    from .rgbd_pose import pose_recovery_ransac_rgbd_batched

    hyp, B, dist, img = _rgbd_args(outputs, real_K, inlier_dist, image_index)
    return _rgbd_shaped(pose_recovery_ransac_rgbd_batched(*pnp_inputs(outputs, real_K), depth, dist, img, **kw), hyp, B)


def rgbd_for_outputs_async(outputs, real_K, depth, inlier_dist, image_index=None, **kw):
    """rgbd_for_outputs without the host wait -> handle; `rgbd_collect(handle, hyp, B)` reads it.  **kw also takes `host` and
    `stream` (rgbd_pose.pose_recovery_ransac_rgbd_batched_async)."""
    from .rgbd_pose import pose_recovery_ransac_rgbd_batched_async

    hyp, B, dist, img = _rgbd_args(outputs, real_K, inlier_dist, image_index)
    return pose_recovery_ransac_rgbd_batched_async(*pnp_inputs(outputs, real_K), depth, dist, img, **kw)


def rgbd_collect(handle, hyp, B):
    return _rgbd_shaped(handle.result(), hyp, B)


def _check_rgbd(depth, depth_scale, rgbd_inlier_dist):
    """The depth arguments of infer_batch / infer_image, before any device work -> True when the RGB-D solver runs."""
    if depth is None:
        if depth_scale is not None or rgbd_inlier_dist is not None:
            raise ValueError("depth_scale and rgbd_inlier_dist go with a depth image: depth is None")
        return False
    if rgbd_inlier_dist is None:
        raise ValueError("depth needs rgbd_inlier_dist: the inlier radius of the RGB-D solver, in the unit of the network's 3-D points "
                         "(it has no default)")
    if getattr(depth, "ndim", 0) not in (2, 3) or (depth.ndim == 3 and depth.shape[0] != 1):
        raise ValueError(f"depth must be one (dH, dW) image, got shape {tuple(getattr(depth, 'shape', ()))}")
    return True


def _rank_hypotheses(stage2, rot, tvec, ratio, ok, hyp, rgbd=None):
    """run_test.py:168-186 for one mini-batch: per instance the hypotheses sorted by inlier ratio, stage-2 pose where PnP failed.
    rgbd: rgbd_for_outputs' result; every hypothesis then also carries R_rgbd (9,), t_rgbd (3,) (its R, t where the RGB-D solver
    failed), rgbd_inliers_ratio and rgbd_success.  The sort key is the PnP's inlier ratio either way."""
    B = stage2.shape[1]
    results = []
    for b in range(B):
        hyps = []
        for k in range(hyp):
            if ok[k, b]:
                hyps.append(dict(R=rot[k, b], t=tvec[k, b, :, 0], inliers_ratio=float(ratio[k, b]), pnp_success=True))
            else:  # run_test.py:177-179: fall back to the stage-2 pose — float32 as the network returned it (the csv row of
                # such an instance prints float32 values), with the inlier ratio PnP reported
                hyps.append(dict(R=stage2[k, b, :3, :3], t=stage2[k, b, :3, 3], inliers_ratio=float(ratio[k, b]), pnp_success=False))
            if rgbd is not None:
                good = bool(rgbd[3][k, b])
                hyps[-1].update(R_rgbd=(rgbd[0][k, b] if good else np.asarray(hyps[-1]["R"])).reshape(9),
                                t_rgbd=(rgbd[1][k, b, :, 0] if good else np.asarray(hyps[-1]["t"])).reshape(3),
                                rgbd_inliers_ratio=float(rgbd[2][k, b]), rgbd_success=good)
        hyps.sort(key=lambda h: h["inliers_ratio"], reverse=True)                   # run_test.py:186 (stable, like sorted())
        results.append(hyps)
    return results


def _check_on_saturation(on_saturation):
    if on_saturation not in ON_SATURATION:
        raise ValueError(f"on_saturation must be one of {ON_SATURATION}, not {on_saturation!r}")
    return on_saturation == "exact"


def _new_slot(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


def _check_pnp_refine(pnp_refine, pnp_fn):
    check_refine(pnp_refine)
    if pnp_refine is not None and pnp_fn is not None:
        raise ValueError("pnp_refine applies to the batched HIP PnP, not to an injected pnp_fn")


def _pnp_checked(outputs, real_K, slot, pnp_fn, pnp_refine=None):
    """PnP of a forward whose saturation snapshot is `slot` -> ((rot, tvec, ratio, ok), saturated)."""
    if pnp_fn is None:
        *res, saturated = pnp_for_outputs(outputs, real_K, sat_slot=slot, pnp_refine=pnp_refine)
        return tuple(res), saturated
    return pnp_fn(outputs, real_K), bool(slot.item())       # (an injected PnP: the slot is read on its own)


def _forward_exact(net, end_points, hyp, pnp_fn=None, pnp_refine=None):
    """The fallback: one mini-batch again, alone (no look-ahead), in strict fp32 -> (outputs, (rot, tvec, ratio, ok)).  The mode is the
    model's own for this call (Net.precision): the global ops.PRECISION is not touched.  Its PnP refines as the batch's would (pnp_refine)."""
    net.range_fallbacks += 1
    prev = net.precision, net.match_mode
    net.precision, net.match_mode = "f32", "exact"
    try:
        outputs = net(end_points, hyp)
    finally:
        net.precision, net.match_mode = prev
    dev = end_points["real_rgb"].device
    pnp, saturated = _pnp_checked(outputs, end_points["real_K"], ops.saturation_take(dev, _new_slot(dev)), pnp_fn, pnp_refine)
    if saturated:      # (fp32 has no operand format to leave: nothing is left to fall back to)
        raise ops.saturation_error("the strict-fp32 re-run of a mini-batch")
    return outputs, pnp


def infer_batch(net, end_points, hyp=5, pnp_fn=None, on_saturation="raise", pnp_refine=None, depth=None, depth_scale=None,
                rgbd_inlier_dist=None, depth_unit="m"):
    """-> per-instance pose hypotheses sorted by inlier ratio (run_test.py:168-186):
    list over instances of list over hypotheses of dict(R (3,3), t (3,), inliers_ratio, pnp_success).
    pnp_fn(outputs, real_K) -> (rot (hyp,B,3,3), tvec (hyp,B,3,1), ratio (hyp,B), ok (hyp,B)) replaces the batched HIP
    PnP (tests of the loop semantics inject canned answers).
    on_saturation: "raise" | "exact" (module docstring): with "exact" a forward that clamped an operand is run again in strict fp32.
    pnp_refine: None | "lm" (module docstring): the poses are refined on their consensus sets; the hypothesis order stays the inlier
    ratio's of pnp_refine=None.  ValueError, before any device work, for another value or with pnp_fn.
    depth: the test depth image (dH, dW) of the batch's instances — float in the network's unit (metres; depth_unit="mm" for float
    millimetres) or uint16 raw with depth_scale (millimetres per unit) — with rgbd_inlier_dist, the inlier radius of the RGB-D
    solver in the network's unit (a number or one per instance; no default: ValueError without it).  Every hypothesis then also
    carries R_rgbd (9,), t_rgbd (3,) (the unit of t; equal to R, t where rgbd_success is false), rgbd_inliers_ratio and
    rgbd_success; everything else, the order included, is the result of a call without depth."""
    _check_pnp_refine(pnp_refine, pnp_fn)
    with_depth = _check_rgbd(depth, depth_scale, rgbd_inlier_dist)
    if not _check_on_saturation(on_saturation):
        outputs = net(end_points, hyp)
        if pnp_fn is not None:
            rot, tvec, ratio, ok = pnp_fn(outputs, end_points["real_K"])
        else:
            rot, tvec, ratio, ok = pnp_for_outputs(outputs, end_points["real_K"], pnp_refine=pnp_refine)
    else:
        dev = end_points["real_rgb"].device
        ops.saturation_word(dev)            # (registered before the first producer of this device runs)
        net._query_stash = None             # this forward computes its own query ViT: the snapshot then covers all of this batch
        outputs = net(end_points, hyp)
        (rot, tvec, ratio, ok), saturated = _pnp_checked(outputs, end_points["real_K"], ops.saturation_take(dev, _new_slot(dev)), pnp_fn,
                                                         pnp_refine)
        if saturated:
            outputs, (rot, tvec, ratio, ok) = _forward_exact(net, end_points, hyp, pnp_fn, pnp_refine)
    rgbd = None
    if with_depth:
        rgbd = rgbd_for_outputs(outputs, end_points["real_K"], depth, rgbd_inlier_dist, depth_scale=depth_scale, depth_unit=depth_unit)
    stage2 = np.stack([o["pred_poses"].cpu().numpy() for o in outputs])            # (hyp,B,4,4) float32
    return _rank_hypotheses(stage2, rot, tvec, ratio, ok, hyp, rgbd)


def infer_image(net, data, templates_data, hyp=5, bs=16, pnp_fn=None, pipelined=True, next_data=None, on_saturation="raise",
                indexed_bank=False, pnp_refine=None, depth=None, depth_scale=None, rgbd_inlier_dist=None, depth_unit="m"):
    """One test image exactly as run_test.py:141-188 walks it: `data` holds the image's instances on dim 1
    (data[key][0] = (n_instance, ...), plus 'obj_idx'), `templates_data[key]` the per-object template bank
    ((n_objects, N, ...), including 'template_feature' and, optionally, an extended bank under 'template_cache').
    Instances are processed in mini-batches of `bs`; returns preds_image: per instance the hypotheses sorted by
    inlier ratio, each {'R_stage_3' (9,), 't_stage_3' (3,) in mm, 'inliers_ratio'} (run_test.py:181-186).
    pipelined (default; HIP PnP only): the mini-batches of an image are independent, so mini-batch j + 1's forward is launched
    BEFORE the host waits for mini-batch j's PnP results (its PnP launch + device->host copy are already enqueued behind its forward) —
    the card does not idle while the host ranks hypotheses; same results, same order.  pipelined=False: the reference's strictly
    sequential walk (every mini-batch ends with a host wait).
    next_data: the NEXT test image's `data` (an evaluator's loader has it one iteration ahead): the query crops of its first mini-batch
    ride in this image's last forward, as the mini-batches of one image do among themselves — same results.
    on_saturation: "raise" (default) | "exact" (module docstring), for both walks.  With "exact" no forward carries another mini-batch's query
    crops (and next_data is not used): the snapshot taken after a forward is then that mini-batch's own verdict, and a batch re-run in
    fp32 leaves no look-ahead behind that a later batch would have consumed.  The pipelined walk still launches mini-batch j + 1 before
    it reads mini-batch j; a flagged j is re-run synchronously when it is read, and preds_image keeps the instance order.
    indexed_bank: the per-object tensors of `templates_data` go to the network as they are, and each instance names its object
    (end_points["template_index"] = its obj_idx): no copy of the bank per instance (run_test.py:159-162 makes one: ~308 MB per detection at
    ViT-L, 162 views), and a template shared by several instances is streamed once by stage 1.  Same results as the default.
    pnp_refine: None | "lm" (module docstring), for both walks and for the strict-fp32 re-runs; the hypothesis order does not change.
    depth, depth_scale, depth_unit, rgbd_inlier_dist: the image's depth image and the RGB-D solver's inlier radius, as infer_batch
    (rgbd_inlier_dist a number or one per instance); every hypothesis then also holds 'R_rgbd' (9,), 't_rgbd' (3,) in mm,
    'rgbd_inliers_ratio' and 'rgbd_success'.  The depth is converted on the device once per image."""
    _check_pnp_refine(pnp_refine, pnp_fn)
    exact = _check_on_saturation(on_saturation)
    with_depth = _check_rgbd(depth, depth_scale, rgbd_inlier_dist)
    n_instance = data["score"].shape[1]
    preds_image = []
    if with_depth and n_instance > 0:
        from .rgbd_pose import depth_on_device

        if np.ndim(rgbd_inlier_dist) != 0 and tuple(np.shape(rgbd_inlier_dist)) != (n_instance,):
            raise ValueError(f"rgbd_inlier_dist must be a number or one per instance ({n_instance},), got shape {tuple(np.shape(rgbd_inlier_dist))}")
        depth = depth_on_device(depth, data["real_rgb"].device, depth_scale, depth_unit)     # float32 metres from here on
    dist_of = lambda start, end: rgbd_inlier_dist if np.ndim(rgbd_inlier_dist) == 0 else rgbd_inlier_dist[start:end]  # noqa: E731

    def inputs_of(start, end):
        obj_idx = data["obj_idx"][0][start:end].reshape(-1)
        inputs = {k: v[0][start:end].contiguous() for k, v in data.items() if v[0].dim() > 0}
        if indexed_bank:
            obj_idx = obj_idx.long()
            inputs["template_index"] = obj_idx
        for k, v in templates_data.items():
            if k == "template_cache":   # extended bank: maps stay per object, instances carry their object index
                inputs[k] = {"obj_index": obj_idx, "dpt": v["dpt"]}
            else:
                inputs[k] = v if indexed_bank else v[obj_idx].contiguous()
        return inputs

    def emit(batch_results):
        for hyps in batch_results:
            preds_image.append([{"R_stage_3": np.asarray(h["R"]).reshape(9), "t_stage_3": np.asarray(h["t"]).reshape(3) * 1000,
                                 "inliers_ratio": h["inliers_ratio"]} for h in hyps])
            if with_depth:
                for out, h in zip(preds_image[-1], hyps):
                    out.update(R_rgbd=h["R_rgbd"], t_rgbd=h["t_rgbd"] * 1000, rgbd_inliers_ratio=h["rgbd_inliers_ratio"],
                               rgbd_success=h["rgbd_success"])

    if pnp_fn is not None or not pipelined:
        for start in range(0, n_instance, bs):
            end = min(start + bs, n_instance)
            rgbd_kw = dict(depth=depth, rgbd_inlier_dist=dist_of(start, end)) if with_depth else {}
            emit(infer_batch(net, inputs_of(start, end), hyp, pnp_fn=pnp_fn, on_saturation=on_saturation, pnp_refine=pnp_refine, **rgbd_kw))
        return preds_image
    pending = None      # (PnP handle, pinned stage-2 poses, their event, batch size, inputs) of the mini-batch in flight
    starts = list(range(0, n_instance, bs))
    if exact and n_instance > 0:
        dev = data["real_rgb"].device
        ops.saturation_word(dev)            # (registered before the first producer of this device runs)
        net._query_stash = None             # (a look-ahead left by an earlier call: this image's first forward computes its own query ViT)
    for j, start in enumerate(starts):
        inputs = inputs_of(start, min(start + bs, n_instance))
        # the next mini-batch's query crops ride in this one's template-side ViT pass (Net.forward_test): same bits, fuller launches
        if exact:
            nxt = None
        elif j + 1 < len(starts):
            nxt = data["real_rgb"][0][starts[j + 1]:min(starts[j + 1] + bs, n_instance)].contiguous()
        elif next_data is not None and next_data["score"].shape[1] > 0:
            nxt = next_data["real_rgb"][0][0:min(bs, next_data["score"].shape[1])].contiguous()
        else:
            nxt = None
        outputs = net(inputs, hyp, next_real_rgb=nxt) if nxt is not None else net(inputs, hyp)
        slot = ops.saturation_take(dev, _new_slot(dev)) if exact else None       # this forward's verdict, in stream order
        handle = pnp_for_outputs_async(outputs, inputs["real_K"], sat_slot=slot, pnp_refine=pnp_refine)
        rgbd = None     # (RGB-D handle, depth, inlier radius): the launch rides behind the PnP's, read when the PnP is
        if with_depth:
            dist = dist_of(start, min(start + bs, n_instance))
            rgbd = (rgbd_for_outputs_async(outputs, inputs["real_K"], depth, dist), depth, dist)
        s2 = torch.stack([o["pred_poses"] for o in outputs])                        # (hyp,B,4,4) float32
        s2_host = torch.empty(s2.shape, dtype=s2.dtype, pin_memory=True)
        s2_host.copy_(s2, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        if pending is not None:
            emit(_collect(pending, hyp, net, pnp_refine))
        pending = (handle, s2_host, ev, s2.shape[1], inputs if exact else None, rgbd)
    if pending is not None:
        emit(_collect(pending, hyp, net, pnp_refine))
    return preds_image


ASSEMBLE_KEYS = ("scene_id", "img_id", "seg_filter_score", "img_size", "pts_size", "minimum_n_point", "rgb_mask_flag", "device", "stream")


def infer_detections(net, image_u8, detections, K, templates_data, obj_idxs, **kw):
    """One decoded test image and its CNOS detection records -> (preds_image, data): provider.test_batch.assemble_test_image
    (the keywords of ASSEMBLE_KEYS go there; scene_id and img_id are required), then infer_image on its `data` with the
    remaining keywords.  ([], None) when no detection passes the score filter."""
    from .provider.test_batch import assemble_test_image

    data = assemble_test_image(image_u8, detections, K, obj_idxs, **{k: kw.pop(k) for k in ASSEMBLE_KEYS if k in kw})
    if data is None:
        return [], None
    return infer_image(net, data, templates_data, **kw), data


LABEL_KEYS = ("topk", "min_score", "max_detections", "nms_iou", "min_area_px", "time", "appearance", "appearance_weight")       # label_proposals' own
LABEL_SHARED_KEYS = ("scene_id", "img_id", "img_size", "minimum_n_point", "bs", "device")       # ... and those both steps read


def infer_proposals(net, image_u8, proposals, K, templates_data, bank, **kw):
    """One decoded test image and a class-agnostic segmenter's mask proposals -> (preds_image, data, detections):
    proposals.label_proposals against `bank` (proposals.describe_templates of the same `templates_data`, in the same object order:
    object id bank.obj_ids[o] is bank row o of `templates_data`), then infer_detections on the labelled records.  The keywords of
    LABEL_KEYS go to label_proposals, those of LABEL_SHARED_KEYS to both steps, every other one to infer_detections —
    `rgb_mask_flag` among them, which is the pose network's there (the labelling keeps its own default: masked crops).
    detections: the records, best first, one per entry of preds_image.  ([], None, []) when no proposal survives the labelling or
    the score filter."""
    from .proposals import label_proposals

    lkw = {k: kw.pop(k) for k in LABEL_KEYS if k in kw}
    lkw.update({k: kw[k] for k in LABEL_SHARED_KEYS if k in kw})
    detections = label_proposals(net, image_u8, proposals, bank, **lkw)
    if not detections:
        return [], None, []
    obj_idxs = {obj_id: o for o, obj_id in enumerate(bank.obj_ids)}
    preds_image, data = infer_detections(net, image_u8, detections, K, templates_data, obj_idxs, **kw)
    if data is None:
        return [], None, []
    kept = [d for d in detections if d["score"] > kw.get("seg_filter_score", 0.0)]
    return preds_image, data, kept


DEPTH_PROPOSAL_KEYS = ("tau", "n_hyp", "seed", "min_inliers", "min_height", "max_height", "max_range", "max_step", "max_area_frac",
                       "drop_border", "max_proposals")       # depth_proposals' own (min_area_px stays label_proposals', see below)


def infer_depth_proposals(net, image_u8, depth, K, templates_data, bank, **kw):
    """One decoded test image and its depth image (H, W) -> (preds_image, data, detections, proposals): depth_proposals.depth_proposals
    segments the depth image (the project's own depth clusterer; the keywords of DEPTH_PROPOSAL_KEYS go there, `proposal_min_area_px`
    as its min_area_px, `device` to both), then infer_proposals labels the masks against `bank` and estimates the poses.  depth: uint16
    raw with `depth_scale`, or float millimetres.  With `rgbd_inlier_dist` the depth image and `depth_scale` are forwarded too (float
    depth as depth_unit "mm"), so the RGB-D keywords of infer_image keep working; without it the poses are RGB only.  Every other
    keyword is infer_proposals'.  proposals: the segmenter's list, largest first; ([], None, [], proposals) when none survives."""
    from .depth_proposals import depth_proposals

    dkw = {k: kw.pop(k) for k in DEPTH_PROPOSAL_KEYS if k in kw}
    if "proposal_min_area_px" in kw:
        dkw["min_area_px"] = kw.pop("proposal_min_area_px")
    if "device" in kw:
        dkw["device"] = kw["device"]
    if getattr(depth, "ndim", 0) != 2:
        raise ValueError(f"depth must be one (H, W) image, got shape {tuple(getattr(depth, 'shape', ()))}")
    depth_scale = kw.pop("depth_scale", None)
    if depth_scale is None and kw.get("depth_unit", "mm") != "mm":
        raise ValueError("float depth is millimetres here: depth_unit must be 'mm'")
    K33 = np.asarray(K.cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64).reshape(3, 3)      # (a flat list of 9, as BOP stores it)
    proposals = depth_proposals(depth, K33, depth_scale=depth_scale, **dkw)
    if kw.get("rgbd_inlier_dist") is not None:
        kw.update(depth=depth, depth_scale=depth_scale)
        if depth_scale is None:
            kw["depth_unit"] = "mm"
    else:
        kw.pop("depth_unit", None)
    return (*infer_proposals(net, image_u8, proposals, K, templates_data, bank, **kw), proposals)


def _collect(pending, hyp, net, pnp_refine=None):
    handle, s2_host, ev, B, inputs, rgbd = pending
    rot, tvec, ratio, ok = pnp_collect(handle, hyp, B)
    ev.synchronize()
    if handle.saturated:    # (on_saturation="exact" only: the snapshot of this mini-batch's forward was set)
        outputs, (rot, tvec, ratio, ok) = _forward_exact(net, inputs, hyp, pnp_refine=pnp_refine)
        if rgbd is not None:    # (the RGB-D poses of the re-run's correspondences)
            rgbd = rgbd_for_outputs(outputs, inputs["real_K"], rgbd[1], rgbd[2])
        return _rank_hypotheses(np.stack([o["pred_poses"].cpu().numpy() for o in outputs]), rot, tvec, ratio, ok, hyp, rgbd)
    return _rank_hypotheses(s2_host.numpy(), rot, tvec, ratio, ok, hyp, rgbd_collect(rgbd[0], hyp, B) if rgbd is not None else None)


STAGES = {"stage_3": ("R_stage_3", "t_stage_3"), "depth": ("R_depth", "t_depth"), "rgbd": ("R_rgbd", "t_rgbd")}
REFINE_STARTS = ("stage_3", "rgbd")


def bop_csv_lines(scene_id, img_id, obj_ids, scores, preds_image, image_time, stage="stage_3"):
    """The BOP results rows of run_test.py:191-206: one line per instance, best hypothesis, t in millimetres.
    stage: "stage_3" (default) writes the network's pose, "depth" the depth-refined one (refine_predictions must have run: an
    instance whose best hypothesis holds no R_depth is a ValueError), "rgbd" the RGB-D solver's (infer_image with a depth image;
    the same error when the hypothesis holds no R_rgbd)."""
    if stage not in STAGES:
        raise ValueError(f"stage must be one of {sorted(STAGES)}, got {stage!r}")
    kr, kt = STAGES[stage]
    lines = []
    for k, preds in enumerate(preds_image):
        if kr not in preds[0]:
            raise ValueError(f"instance {k}: its best hypothesis holds no {kr!r}; run refine_predictions first"
                             if stage != "rgbd" else f"instance {k}: its best hypothesis holds no {kr!r}; run infer_image with depth first")
        lines.append(",".join((str(scene_id), str(img_id), str(obj_ids[k]), str(scores[k]),
                               " ".join(str(v) for v in preds[0][kr]),
                               " ".join(str(v) for v in preds[0][kt]), f"{image_time}\n")))
    return lines


def suppress_duplicate_poses(rows, models, nms_dist=0.1):
    """Drop the duplicate poses of an image's or a dataset's results (pose_detection_eval.pose_nms: per image and object, by descending
    score, an estimate within nms_dist x diameter — MSSD, symmetries included — of an earlier KEPT one is dropped).  rows: the
    `scene_id,im_id,obj_id,score,R,t,time` content bop_csv_lines prints, as a list of lines (several images' lists concatenated; a
    header line is kept) or as evaluation.read_bop_results' dict; models: an evaluation.ObjectModels.  -> the kept lines, in order, or
    the dict of the kept rows.  The project's own rule: nms_dist = 0.1 is not tuned and its effect on real data is unmeasured; no
    default path of the pipeline calls this."""
    from .evaluation import read_bop_results
    from .pose_detection_eval import pose_nms

    if isinstance(rows, dict):
        keep = pose_nms(rows, models, nms_dist=nms_dist)
        return {k: np.asarray(v)[keep] for k, v in rows.items()}
    lines = list(rows)
    data = [n for n, line in enumerate(lines) if line.strip() and not line.strip().startswith("scene_id")]   # read_bop_results' rule
    kept = {data[k] for k in pose_nms(read_bop_results(lines), models, nms_dist=nms_dist).tolist()}
    blank = set(range(len(lines))) - set(data)
    return [line for n, line in enumerate(lines) if n in kept or n in blank]


def refine_predictions(preds_image, models, obj_ids, K, depth, depth_scale=None, hypotheses="best", rank_by="inliers_ratio",
                       start="stage_3", **kw):
    """Depth refinement of one image's predictions (depth_refine.refine_poses_depth, ONE call for the whole image) -> a new
    preds_image; the input is not modified.  preds_image: infer_image's result; obj_ids: the object id of each instance (ids known
    to `models`, an evaluation.ObjectModels with faces); K (3, 3); depth (H, W) or (1, H, W), uint16 raw with `depth_scale` or float
    millimetres; **kw: refine_poses_depth's parameters.
    hypotheses: "best" refines each instance's first hypothesis, "all" every one.  A refined hypothesis gains 'R_depth' (9,),
    't_depth' (3,) in mm (float32; the input pose where depth_status >= 2), 'depth_status' and 'depth_rms' (rms_after).
    rank_by: "inliers_ratio" keeps the order; "depth" (with "all") re-sorts each instance's hypotheses, stably: those with
    depth_status <= 1 first, in ascending depth_rms, then the others in their order.  ValueError before any device work for another
    value, rank_by="depth" without "all", or obj_ids that do not match preds_image.
    start: "stage_3" (default) refines the network's pose, "rgbd" the RGB-D solver's ('R_rgbd', 't_rgbd' of infer_image with a depth
    image: a start whose translation is already metric).  ValueError for another value, or for "rgbd" when a hypothesis to refine
    holds no 'R_rgbd'."""
    from .depth_refine import refine_poses_depth

    if not (isinstance(start, str) and start in REFINE_STARTS):
        raise ValueError(f"start must be one of {REFINE_STARTS}, got {start!r}")
    kr, kt = STAGES[start]

    if hypotheses not in ("best", "all"):
        raise ValueError(f"hypotheses must be 'best' or 'all', got {hypotheses!r}")
    if rank_by not in ("inliers_ratio", "depth"):
        raise ValueError(f"rank_by must be 'inliers_ratio' or 'depth', got {rank_by!r}")
    if rank_by == "depth" and hypotheses != "all":
        raise ValueError("rank_by='depth' compares an instance's hypotheses: it needs hypotheses='all'")
    if len(obj_ids) != len(preds_image):
        raise ValueError(f"obj_ids must hold one id per instance: {len(obj_ids)} ids for {len(preds_image)} instances")
    if getattr(depth, "ndim", 0) == 2:
        depth = depth[None]
    if getattr(depth, "ndim", 0) != 3 or depth.shape[0] != 1:
        raise ValueError(f"depth must be one (H, W) image, got shape {tuple(getattr(depth, 'shape', ()))}")
    where = [(i, h) for i, hyps in enumerate(preds_image) for h in range(len(hyps) if hypotheses == "all" else min(1, len(hyps)))]
    for i, h in where:
        if kr not in preds_image[i][h]:
            raise ValueError(f"instance {i}, hypothesis {h} holds no {kr!r}: start={start!r} needs infer_image with a depth image")
    R = np.array([np.asarray(preds_image[i][h][kr], dtype=np.float64).reshape(3, 3) for i, h in where]).reshape(-1, 3, 3)
    t = np.array([np.asarray(preds_image[i][h][kt], dtype=np.float64).reshape(3) for i, h in where]).reshape(-1, 3)
    ids = np.array([int(obj_ids[i]) for i, _ in where], dtype=np.int64)
    res = refine_poses_depth(models, ids, R, t, K, depth, depth_scale=depth_scale, **kw)
    Rd, td = res["R"].cpu().numpy().reshape(-1, 9), res["t"].cpu().numpy()
    status, rms = res["status"].cpu().numpy(), res["rms_after"].cpu().numpy()
    out = [[dict(h) for h in hyps] for hyps in preds_image]
    for n, (i, h) in enumerate(where):
        out[i][h].update(R_depth=Rd[n], t_depth=td[n], depth_status=int(status[n]), depth_rms=float(rms[n]))
    if rank_by == "depth":
        for hyps in out:
            hyps.sort(key=lambda h: (0, h["depth_rms"]) if h["depth_status"] <= 1 else (1, 0.0))
    return out


VERIFY_KEYS = ("verify_score", "verify_iou", "verify_visible_iou", "verify_agreement", "verify_counts")


def verify_predictions(preds_image, models, obj_ids, K, segmentations, size, depth=None, depth_scale=None, stage="stage_3",
                       hypotheses="all", rank=True, **kw):
    """Render-and-compare verification of one image's predictions (verify.verify_poses, ONE call for the whole image, mask_index =
    the instance) -> a new preds_image; the input is not modified.  preds_image: infer_image's result; obj_ids: the object id of
    each instance (ids known to `models`, an evaluation.ObjectModels with faces); K (3, 3); segmentations: the COCO-RLE mask of each
    instance, in instance order, each of size = (H, W) — for infer_detections these are the `segmentation`s of the records
    provider.test_batch.select_detections keeps (score > seg_filter_score), in their order; depth: None (RGB only) or one (H, W) or
    (1, H, W) image, uint16 raw with `depth_scale` or float millimetres; **kw: verify_poses' parameters (delta, near, window,
    workspace_bytes).
    stage: the pose that is verified, read through STAGES as refine_predictions reads it (millimetres): "stage_3" (default), "depth"
    or "rgbd"; ValueError when a hypothesis to verify holds no such key.  hypotheses: "all" (default) verifies every hypothesis,
    "best" each instance's first.  A verified hypothesis gains the VERIFY_KEYS: 'verify_score', 'verify_iou', 'verify_visible_iou',
    'verify_agreement' (floats) and 'verify_counts' (8 ints, verify.COUNTS).
    rank=True (needs hypotheses="all") re-sorts each instance's hypotheses by descending verify_score; the sort is stable, so ties
    keep the inlier-ratio order, and bop_csv_lines then prints the verified best hypothesis without change.
    The score is the project's own rule (verify.py's docstring): with modal masks the RGB-only value ranks the hypotheses of one
    instance but is not comparable across instances, and accuracy on real data is unmeasured and not claimed.
    ValueError before any device work: another stage or hypotheses value, rank=True without "all", obj_ids or segmentations that do
    not match preds_image, a depth that is not one image, and verify_poses' own."""
    from .verify import verify_poses

    if not (isinstance(stage, str) and stage in STAGES):
        raise ValueError(f"stage must be one of {sorted(STAGES)}, got {stage!r}")
    kr, kt = STAGES[stage]
    if hypotheses not in ("best", "all"):
        raise ValueError(f"hypotheses must be 'best' or 'all', got {hypotheses!r}")
    if not isinstance(rank, (bool, np.bool_)):
        raise ValueError(f"rank must be a bool, got {rank!r}")
    if rank and hypotheses != "all":
        raise ValueError("rank=True compares an instance's hypotheses: it needs hypotheses='all'")
    if len(obj_ids) != len(preds_image):
        raise ValueError(f"obj_ids must hold one id per instance: {len(obj_ids)} ids for {len(preds_image)} instances")
    if len(segmentations) != len(preds_image):
        raise ValueError(f"segmentations must hold one mask per instance: {len(segmentations)} masks for {len(preds_image)} instances")
    if depth is not None:
        if getattr(depth, "ndim", 0) == 2:
            depth = depth[None]
        if getattr(depth, "ndim", 0) != 3 or depth.shape[0] != 1:
            raise ValueError(f"depth must be one (H, W) image, got shape {tuple(getattr(depth, 'shape', ()))}")
    where = [(i, h) for i, hyps in enumerate(preds_image) for h in range(len(hyps) if hypotheses == "all" else min(1, len(hyps)))]
    for i, h in where:
        if kr not in preds_image[i][h]:
            raise ValueError(f"instance {i}, hypothesis {h} holds no {kr!r}: stage={stage!r} has not run for it")
    R = np.array([np.asarray(preds_image[i][h][kr], dtype=np.float64).reshape(3, 3) for i, h in where]).reshape(-1, 3, 3)
    t = np.array([np.asarray(preds_image[i][h][kt], dtype=np.float64).reshape(3) for i, h in where]).reshape(-1, 3)
    ids = np.array([int(obj_ids[i]) for i, _ in where], dtype=np.int64)
    res = verify_poses(models, ids, R, t, K, segmentations, size, mask_index=np.array([i for i, _ in where], dtype=np.int64),
                       depth=depth, depth_scale=depth_scale, **kw)
    host = {k: res[k].cpu().numpy() for k in ("score", "iou", "visible_iou", "agreement", "counts")}
    out = [[dict(h) for h in hyps] for hyps in preds_image]
    for n, (i, h) in enumerate(where):
        out[i][h].update(verify_score=float(host["score"][n]), verify_iou=float(host["iou"][n]),
                         verify_visible_iou=float(host["visible_iou"][n]), verify_agreement=float(host["agreement"][n]),
                         verify_counts=[int(c) for c in host["counts"][n]])
    if rank:
        for hyps in out:
            hyps.sort(key=lambda h: -h["verify_score"])
    return out
