"""Host mirror of reference utils/pose_recovery.py (HIP through the C ABI).

Opt-in pose refinement (refine="lm"): the batched PnP launch runs a Levenberg-Marquardt tail on each problem's RANSAC consensus
set (pp_pnp_ransac_refine: the cv2.solvePnPRefineLM step OpenCV users add after cv2.solvePnPRansac).  It moves R and t only:
the consensus (inliers_ratio), success and npts — and so the ranking of hypotheses by inlier ratio — are those of refine=None,
which makes exactly the launch and the device->host copy it made before the option existed."""
import numbers
import os

import torch

from .. import _lib

REFINE_MODES = (None, "lm")
REFINE_EPS = 2.0 ** -23          # FLT_EPSILON: the tolerance of cv2.solvePnPRefineLM's default criteria (with 20 iterations)
MAX_POINTS = 4096                # correspondences per problem (include/picopose_hip.h)


def check_refine(refine, refine_iters=20, refine_eps=REFINE_EPS, return_inliers=False):
    """Validate the refinement arguments before any device work -> True when refining.  ValueError for a mode other than
    None / "lm", a refine_iters that is not a positive integer, a refine_eps that is negative or not a finite number, and
    return_inliers without refinement (the consensus mask is an output of the refining launch only)."""
    if not (refine is None or (isinstance(refine, str) and refine in REFINE_MODES)):
        raise ValueError(f"refine must be one of {REFINE_MODES}, not {refine!r}")
    if isinstance(refine_iters, bool) or not isinstance(refine_iters, numbers.Integral) or refine_iters <= 0:
        raise ValueError(f"refine_iters must be a positive integer, not {refine_iters!r}")
    if isinstance(refine_eps, bool) or not isinstance(refine_eps, numbers.Real) or not 0.0 <= float(refine_eps) < float("inf"):
        raise ValueError(f"refine_eps must be a finite number >= 0, not {refine_eps!r}")
    if return_inliers and refine is None:
        raise ValueError("return_inliers needs refine='lm': the consensus mask is an output of the refining launch")
    return refine is not None


def pose_recovery_2d_prediction(query_M, query_K, pred_Ms, template_K, template_Ms, template_poses):
    """Drop-in for reference utils/pose_recovery.py:9-65 -> pred_poses (B,4,4).

    The reference asserts, with two host syncs per call, that query_M is a crop affine (M01 = M10 = 0, M00 = M11:
    `inverse_affine`, torch_utils.py:100-101).  Here that is the caller's contract by default — the path stays
    sync-free — and PP_CHECK_CONTRACTS=1 in the environment restores the two asserts (same AssertionError)."""
    qM, qK, pM, tK, tM, tp = _lib.dev_f32(query_M, query_K, pred_Ms, template_K, template_Ms, template_poses)
    if os.environ.get("PP_CHECK_CONTRACTS") == "1":
        assert torch.all(qM[:, 0, 1] == 0) and torch.all(qM[:, 1, 0] == 0)          # torch_utils.py:100
        assert torch.all(qM[:, 0, 0] == qM[:, 1, 1])                                 # torch_utils.py:101
    B = qM.shape[0]
    out = torch.empty(B, 4, 4, dtype=torch.float32, device=qM.device)
    _lib.call("pp_pose_recovery_2d", qM, qK, pM, tK, tM, tp, B, out)
    return out


def alloc_pose_outputs(P, dev):
    """The outputs every batched RANSAC launch (PnP, RGB-D) writes -> rot (P,3,3) f64, tvec (P,3) f64, ratio (P) f64, ok (P) i32,
    npts (P) i32, uninitialised on `dev`."""
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    return torch.empty(P, 3, 3, **f64), torch.empty(P, 3, **f64), torch.empty(P, **f64), torch.empty(P, **i32), torch.empty(P, **i32)


def launch_and_copy_async(launch, pack, stream=None, stream_inputs=(), host=None, mask_at=None):
    """The asynchronous tail of a batched RANSAC launch (PnP, RGB-D) -> (host, event, P, mask).  launch() enqueues the kernel and
    returns its device tensors, pack(launched) makes the ONE (P [+ 1], columns) f64 device tensor that travels: it is copied into a
    pinned buffer (`host`, reused when its shape fits) without a host wait, launched[mask_at] (uint8, if asked for) into a second
    one, and the event is recorded behind both.  stream: a side stream for all of it; it first waits for the current stream, and
    the caching allocator must not hand out the blocks of `stream_inputs` while the side stream reads them."""
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        for t in stream_inputs:
            t.record_stream(stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        launched = launch()
        packed = pack(launched)
        if host is None or tuple(host.shape) != tuple(packed.shape):
            host = torch.empty(tuple(packed.shape), dtype=torch.float64, pin_memory=True)
        host.copy_(packed, non_blocking=True)
        mask = None
        if mask_at is not None:
            mask = torch.empty(tuple(launched[mask_at].shape), dtype=torch.uint8, pin_memory=True)
            mask.copy_(launched[mask_at], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
    return host, ev, launched[0].shape[0], mask


def pnp_launch(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, iterations=150, reproj_error=2.0, branches=False, refine=None,
               refine_iters=20, refine_eps=REFINE_EPS, return_inliers=False):
    """Enqueue the batched PnP/RANSAC kernel; returns DEVICE tensors (rot (P,3,3) f64, tvec (P,3) f64, ratio (P) f64,
    ok (P) i32, npts (P) i32 = correspondences each problem received) without synchronising.  branches=True: a sixth tensor
    (P,40) f64, the refit's three beta-branch candidates [R, t, error] and the index of the one kept (pp_pnp_ransac_debug).
    refine="lm": pp_pnp_ransac_refine — rot / tvec are the refined poses (ratio, ok and npts are refine=None's) and three more
    tensors follow: rms_before, rms_after (P) f64 (px, over the consensus set) and the accepted LM steps (P) i32; with
    return_inliers a fourth, the consensus mask (P,N) uint8 in the order of the valid entries of tar_pts.  refine_iters /
    refine_eps: the stopping rule of include/picopose_hip.h (cv2.solvePnPRefineLM's defaults)."""
    refining = check_refine(refine, refine_iters, refine_eps, return_inliers)
    if branches and refining:
        raise ValueError("branches (pp_pnp_ransac_debug) instruments the unrefined launch: use refine=None with it")
    t2, s3, Kd, pose = _lib.dev_f32(tar_pts_2d, src_pts_3d, K, tem_pose)
    tp, sp = tar_pts.contiguous().long(), src_pts.contiguous().long()
    P, _, H, W = t2.shape
    N = tp.shape[1]
    dev = t2.device
    rot, tvec, ratio, ok, npts = alloc_pose_outputs(P, dev)
    if branches:
        dbg = torch.empty(P, 40, dtype=torch.float64, device=dev)
        _lib.call("pp_pnp_ransac_debug", t2, s3, Kd, pose, tp, sp, P, H, W, N, int(iterations), float(reproj_error),
                  rot, tvec, ratio, ok, npts, dbg)
        return rot, tvec, ratio, ok, npts, dbg
    if refining:
        rms0 = torch.empty(P, dtype=torch.float64, device=dev)
        rms1 = torch.empty(P, dtype=torch.float64, device=dev)
        its = torch.empty(P, dtype=torch.int32, device=dev)
        mask = torch.empty(P, N, dtype=torch.uint8, device=dev) if return_inliers else None
        _lib.call("pp_pnp_ransac_refine", t2, s3, Kd, pose, tp, sp, P, H, W, N, int(iterations), float(reproj_error),
                  int(refine_iters), float(refine_eps), rot, tvec, ratio, ok, npts, rms0, rms1, its, mask)
        return (rot, tvec, ratio, ok, npts, rms0, rms1, its) + ((mask,) if return_inliers else ())
    _lib.call("pp_pnp_ransac", t2, s3, Kd, pose, tp, sp, P, H, W, N, int(iterations), float(reproj_error), rot, tvec, ratio, ok, npts)
    return rot, tvec, ratio, ok, npts


def refit_branches(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, iterations=150, reproj_error=2.0):
    """Parity instrument (tests): the batched kernel's result plus, per problem, the three beta-branch candidates of its final
    refit -> rot (P,3,3), tvec (P,3,1), ratio (P), ok (P), branches: list (P) of ([(err, R (3,3), t (3,))] * 3, kept index)."""
    rot, tvec, ratio, ok, npts, dbg = pnp_launch(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, iterations, reproj_error,
                                                 branches=True)
    d = dbg.cpu().numpy()
    out = []
    for p in range(d.shape[0]):
        cand = [(float(d[p, 13 * a + 12]) if d[p, 13 * a + 12] < 1e299 else float("inf"), d[p, 13 * a:13 * a + 9].reshape(3, 3).copy(),
                 d[p, 13 * a + 9:13 * a + 12].copy()) for a in range(3)]
        out.append((cand, int(d[p, 39])))
    return rot.cpu().numpy(), tvec.cpu().numpy()[:, :, None], ratio.cpu().numpy(), ok.cpu().numpy() != 0, out


def _packed(launched):
    """The launch's results as ONE (P, 15) f64 device tensor — (P, 18) with the refinement's rms_before, rms_after, iterations."""
    rot, tvec, ratio, ok, npts = launched[:5]
    P = rot.shape[0]
    cols = [rot.reshape(P, 9), tvec, ratio[:, None], ok.double()[:, None], npts.double()[:, None]]
    if len(launched) > 5:
        rms0, rms1, its = launched[5:8]
        cols += [rms0[:, None], rms1[:, None], its.double()[:, None]]
    return torch.cat(cols, dim=1)


def _unpacked(host, P, return_npts):
    """host (P, 15 | 18) -> rot, tvec, ratio, ok [+ npts] [+ refine_stats]."""
    res = (host[:, :9].reshape(P, 3, 3).copy(), host[:, 9:12].reshape(P, 3, 1).copy(), host[:, 12].copy(), host[:, 13] != 0)
    res = res + (host[:, 14].astype("int32"),) if return_npts else res
    if host.shape[1] > 15:
        res = res + (dict(rms_before=host[:, 15].copy(), rms_after=host[:, 16].copy(), iterations=host[:, 17].astype("int32")),)
    return res


def pose_recovery_ransac_pnp_batched(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, iterations=150,
                                     reproj_error=2.0, return_npts=False, sat_slot=None, refine=None, refine_iters=20,
                                     refine_eps=REFINE_EPS, return_inliers=False):
    """All (instance, hypothesis) problems of a batch in ONE launch and ONE device->host copy
    (the reference loops over them on the host with a sync each, run_test.py:168-184).

    tar_pts_2d (P,2,H,W), src_pts_3d (P,3,H,W), K (P,3,3), tem_pose (P,4,4), tar_pts/src_pts (P,N,2) int64
    -> rot (P,3,3) f64, tvec (P,3,1) f64, inliers_ratio (P) f64, success (P) bool   (numpy arrays)
    [+ npts (P) int32 with return_npts] [+ refine_stats with refine] [+ inliers with return_inliers] [+ saturated (bool) with sat_slot].
    sat_slot: a forward's saturation snapshot (ops.saturation_take): the copy carries THAT instead of the live word, and a set slot is
    returned as `saturated` instead of raising (the caller recomputes the batch: pipeline.py, on_saturation="exact").
    refine="lm": each pose is refined by Levenberg-Marquardt on its RANSAC consensus set (module docstring; include/picopose_hip.h,
    pp_pnp_ransac_refine).  inliers_ratio, success and npts are exactly those of refine=None; rot and tvec are the refined pose.
    refine_stats = dict(rms_before, rms_after (P) f64 px, iterations (P) int32) rides in the same copy (three more columns).
    return_inliers (refine="lm" only): the consensus mask (P,N) bool in the order of the valid entries of tar_pts (cv2's `inliers`),
    one more copy."""
    launched = pnp_launch(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, iterations, reproj_error, refine=refine,
                          refine_iters=refine_iters, refine_eps=refine_eps, return_inliers=return_inliers)
    P = launched[0].shape[0]
    # one packed device->host copy (P x 15 doubles, 18 when refining, + the saturation row) instead of four
    host = _with_sat_row(_packed(launched), sat_slot).cpu().numpy()
    if sat_slot is not None:
        host, saturated = host[:P], bool(host[P, 0] != 0)
    else:
        host = _check_sat_row(host, P)
    res = _unpacked(host, P, return_npts)
    res = res + (launched[8].cpu().numpy() != 0,) if return_inliers else res
    return res + (saturated,) if sat_slot is not None else res


def _with_sat_row(packed, slot=None):
    """packed (P, 15) f64 on the device + ONE more row whose first entry is the sticky operand-saturation word (picopose_amd/ops.py): the
    host learns with the poses' own copy — no extra synchronisation — whether the forward that produced them clamped an operand.
    slot: carry this snapshot of the word instead (ops.saturation_take; the row is then always there)."""
    from .. import ops

    w = ops.saturation_word(packed.device) if slot is None else slot
    if w is None:
        return packed
    row = torch.zeros(1, packed.shape[1], dtype=packed.dtype, device=packed.device)
    row[0, 0] = w[0]
    return torch.cat([packed, row])


def _check_sat_row(host, P):
    """host (P or P + 1, 15): strips the saturation row; raises (and resets the word) if it is set."""
    if host.shape[0] == P:
        return host
    if host[P, 0] != 0:
        from .. import ops

        ops.saturation_word().zero_()
        raise ops.saturation_error("a forward since the saturation word was last read (sticky: normally the forward whose poses were just read)")
    return host[:P]


class PnPHandle:
    """A batched PnP launch whose result is on its way to the host (pose_recovery_ransac_pnp_batched_async)."""
    __slots__ = ("host", "event", "P", "slot", "saturated", "mask")

    def __init__(self, host, event, P, slot=False, mask=None):
        self.host, self.event, self.P, self.slot, self.saturated, self.mask = host, event, P, slot, None, mask

    def result(self, return_npts=False):
        """Wait for the copy and unpack: rot (P,3,3) f64, tvec (P,3,1) f64, inliers_ratio (P) f64, success (P) bool [+ npts]
        [+ refine_stats of a refining launch] [+ inliers (P,N) bool of a launch with return_inliers].
        A launch with a saturation snapshot (sat_slot) does not raise: `.saturated` tells whether the slot was set."""
        self.event.synchronize()
        P = self.P
        if self.slot:
            host = self.host.numpy()
            host, self.saturated = host[:P], bool(host[P, 0] != 0)
        else:
            host = _check_sat_row(self.host.numpy(), P)
        res = _unpacked(host, P, return_npts)
        return res + (self.mask.numpy() != 0,) if self.mask is not None else res


def pose_recovery_ransac_pnp_batched_async(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, iterations=150, reproj_error=2.0,
                                           host=None, stream=None, sat_slot=None, refine=None, refine_iters=20, refine_eps=REFINE_EPS,
                                           return_inliers=False):
    """pose_recovery_ransac_pnp_batched without the host wait: the launch and ONE asynchronous device->host copy (P x 15 doubles
    into a pinned buffer, `host` to reuse one) are enqueued on the current stream; `.result()` of the returned handle waits for
    them.  A serving loop launches batch i + 1 before it reads batch i's poses, so the GPU never waits for the host.
    stream: a side torch.cuda.Stream for the PnP launch and the copy (it first waits for the current stream, i.e. for the forward
    that produced the inputs): the batch's PnP — one 512-thread workgroup per problem, latency-bound fp64 work on 160 of the
    256 CUs — then runs beside the NEXT batch's forward instead of in front of it.
    sat_slot: the forward's saturation snapshot travels in the copy instead of the live word; `.result()` then reports it as `.saturated`.
    refine / refine_iters / refine_eps / return_inliers: as pose_recovery_ransac_pnp_batched (refining: P x 18 doubles in the copy;
    the mask is a second asynchronous copy)."""
    check_refine(refine, refine_iters, refine_eps, return_inliers)
    inputs = (tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts)
    host, ev, P, mask = launch_and_copy_async(
        lambda: pnp_launch(*inputs, iterations, reproj_error, refine=refine, refine_iters=refine_iters, refine_eps=refine_eps,
                           return_inliers=return_inliers),
        lambda launched: _with_sat_row(_packed(launched), sat_slot), stream,
        inputs + ((sat_slot,) if sat_slot is not None else ()), host, 8 if return_inliers else None)
    return PnPHandle(host, ev, P, slot=sat_slot is not None, mask=mask)


def pose_recovery_ransac_pnp(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, *, refine=None, refine_iters=20,
                             refine_eps=REFINE_EPS, return_inliers=False):
    """Drop-in for reference utils/pose_recovery.py:68-105 (one instance/hypothesis):
    -> (rot ndarray(3,3), tvecs ndarray(3,1), inliers_ratio float, success bool); never raises for bad
    geometry — failure returns (I, [0,0,1]^T, 0.0, False) like the reference's except branch.
    refine="lm" (keyword only; the six positional arguments are the reference's): the pose refined on the consensus set, and a
    fifth element, refine_stats = dict(rms_before, rms_after (px), iterations); inliers_ratio and success are unchanged.
    return_inliers (with refine="lm"): one more element, the consensus mask (N,) bool in the order of the valid entries of tar_pts."""
    check_refine(refine, refine_iters, refine_eps, return_inliers)
    res = pose_recovery_ransac_pnp_batched(tar_pts_2d[None], src_pts_3d[None], K[None], tem_pose[None], tar_pts[None], src_pts[None],
                                           refine=refine, refine_iters=refine_iters, refine_eps=refine_eps,
                                           return_inliers=return_inliers)
    rot, tvec, ratio, ok = res[:4]
    out = (rot[0], tvec[0], float(ratio[0]), bool(ok[0]))
    if refine is not None:
        st = res[4]
        out = out + (dict(rms_before=float(st["rms_before"][0]), rms_after=float(st["rms_after"][0]), iterations=int(st["iterations"][0])),)
    return out + (res[-1][0],) if return_inliers else out


def solve_pnp_refine_lm(object_points, image_points, K, R, t, counts=None, max_iters=20, eps=REFINE_EPS):
    """cv2.solvePnPRefineLM over a ragged batch, on the GPU (pp_pnp_refine_lm; cost, parameters and stopping rule: include/picopose_hip.h).
    object_points (P,Nmax,3), image_points (P,Nmax,2), K (P,3,3) or (3,3), R (P,3,3), t (P,3) or (P,3,1): CUDA tensors, evaluated
    in float64; counts: the rows each problem uses (P,) (default: all Nmax), Nmax <= 4096.  A problem with fewer than 6 points (or a
    non-finite start) keeps its start, with 0 iterations.
    -> rot (P,3,3) f64, tvec (P,3,1) f64, refine_stats = dict(rms_before, rms_after (P) f64 px, iterations (P) int32)  (numpy; one
    device->host copy).  ValueError for bad shapes or arguments, before any device work."""
    check_refine("lm", max_iters, eps)
    shapes = [tuple(x.shape) for x in (object_points, image_points, K, R, t)]
    if len(shapes[0]) != 3 or shapes[0][2] != 3:
        raise ValueError(f"object_points must be (P, Nmax, 3), not {shapes[0]}")
    P, Nmax = shapes[0][:2]
    if P < 1 or not 1 <= Nmax <= MAX_POINTS:
        raise ValueError(f"object_points (P, Nmax, 3) needs P >= 1 and 1 <= Nmax <= {MAX_POINTS}, not {shapes[0]}")
    if shapes[1] != (P, Nmax, 2):
        raise ValueError(f"image_points must be {(P, Nmax, 2)}, not {shapes[1]}")
    if shapes[2] not in ((3, 3), (P, 3, 3)) or shapes[3] != (P, 3, 3) or shapes[4] not in ((P, 3), (P, 3, 1)):
        raise ValueError(f"K (P,3,3) or (3,3), R (P,3,3), t (P,3) or (P,3,1) for P = {P}, not {shapes[2:]}")
    if counts is not None:
        counts = counts if isinstance(counts, torch.Tensor) else torch.as_tensor(counts)
        if tuple(counts.shape) != (P,):
            raise ValueError(f"counts must be ({P},), not {tuple(counts.shape)}")
        if not counts.is_cuda and (int(counts.min()) < 0 or int(counts.max()) > Nmax):
            raise ValueError(f"counts must lie in [0, {Nmax}]")
    for x in (object_points, image_points, K, R, t):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _lib.PicoPoseHipError("picopose_amd runs on the GPU only: inputs must be CUDA(HIP) tensors")
    dev = object_points.device
    f64 = lambda x: x.to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
    obj, img, R0, t0 = f64(object_points), f64(image_points), f64(R), f64(t).reshape(P, 3)
    Kd = f64(K).expand(P, 3, 3).contiguous()
    cnt = (torch.full((P,), Nmax, dtype=torch.int32, device=dev) if counts is None
           else counts.to(device=dev, dtype=torch.int32).contiguous())
    rot = torch.empty(P, 3, 3, dtype=torch.float64, device=dev)
    tvec = torch.empty(P, 3, dtype=torch.float64, device=dev)
    rms0 = torch.empty(P, dtype=torch.float64, device=dev)
    rms1 = torch.empty(P, dtype=torch.float64, device=dev)
    its = torch.empty(P, dtype=torch.int32, device=dev)
    _lib.call("pp_pnp_refine_lm", obj, img, cnt, Kd, R0, t0, P, Nmax, int(max_iters), float(eps), rot, tvec, rms0, rms1, its)
    host = torch.cat([rot.reshape(P, 9), tvec, rms0[:, None], rms1[:, None], its.double()[:, None]], dim=1).cpu().numpy()
    return (host[:, :9].reshape(P, 3, 3).copy(), host[:, 9:12].reshape(P, 3, 1).copy(),
            dict(rms_before=host[:, 12].copy(), rms_after=host[:, 13].copy(), iterations=host[:, 14].astype("int32")))
