"""RGB-D pose recovery: batched 3D-3D RANSAC on the test depth image (csrc/pp_rgbd_pose.hip; the algorithm is stated in
include/picopose_hip.h, "RGB-D POSE RECOVERY", and restated in numpy by tests/rgbd_pose_oracle.py).

    rot, tvec, ratio, ok, npts, stats = pose_recovery_ransac_rgbd_batched(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts,
                                                                          depth, inlier_dist)

Stage 3 gives every (instance, hypothesis) up to ~3 500 pairs of an image pixel and a template 3-D point — the input of the RGB-only
PnP (utils/pose_recovery.py).  Reading the test depth image at the pixel turns each pair into a 3D-3D correspondence, and RANSAC over
three-point rigid fits gives a metric pose directly: its translation along the viewing ray comes from the measured depth, where the
RGB pose is weakest.  One launch serves all problems of a forward; the async form runs it on a side stream without a host wait.

This is the project's own algorithm, held to the numpy restatement.  The project it was modelled on has no RGB-D solver, so there is
no reference parity to claim."""
import numbers

import numpy as np
import torch

from . import _lib
from .scene import depth_u16_scaled
from .utils.pose_recovery import MAX_POINTS, alloc_pose_outputs, launch_and_copy_async

DEPTH_UNITS = {"m": 1.0, "mm": 1e-3}


def _shape(x, name):
    s = getattr(x, "shape", None)
    if s is None:
        raise ValueError(f"{name} must be an array or a tensor, got {type(x).__name__}")
    return tuple(int(v) for v in s)


def _shape_of_values(x, name):
    """Shape of a per-problem argument: a tensor, an array or a (nested) sequence of numbers."""
    try:
        return tuple(int(v) for v in (x.shape if hasattr(x, "shape") else np.shape(x)))
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be numbers, an array or a tensor, got {type(x).__name__}") from None


def check_rgbd_args(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, depth, inlier_dist, image_index=None, iterations=150,
                    depth_scale=None, depth_unit="m"):
    """Validate a batched call before any device work -> (P, H, W, N, n_images, dH, dW).  ValueError for shapes that do not match,
    a missing or malformed inlier_dist, a depth that is not 2-D or 3-D (or whose dtype / depth_scale do not go together), an
    image_index that is not (P,), an iterations that is not a positive integer."""
    s2, s3 = _shape(tar_pts_2d, "tar_pts_2d"), _shape(src_pts_3d, "src_pts_3d")
    if len(s2) != 4 or s2[1] != 2 or 0 in s2:
        raise ValueError(f"tar_pts_2d must be (P, 2, H, W), got {s2}")
    P, _, H, W = s2
    if s3 != (P, 3, H, W):
        raise ValueError(f"src_pts_3d must be {(P, 3, H, W)}, got {s3}")
    if _shape(K, "K") != (P, 3, 3) or _shape(tem_pose, "tem_pose") != (P, 4, 4):
        raise ValueError(f"K must be {(P, 3, 3)} and tem_pose {(P, 4, 4)}, got {_shape(K, 'K')} and {_shape(tem_pose, 'tem_pose')}")
    st, ss = _shape(tar_pts, "tar_pts"), _shape(src_pts, "src_pts")
    if len(st) != 3 or st[0] != P or st[2] != 2 or not 1 <= st[1] <= MAX_POINTS or ss != st:
        raise ValueError(f"tar_pts and src_pts must both be (P, N, 2) with P = {P} and 1 <= N <= {MAX_POINTS}, got {st} and {ss}")
    if inlier_dist is None:
        raise ValueError("inlier_dist is required: the inlier radius in the unit of src_pts_3d (it has no default)")
    if isinstance(inlier_dist, (bool, str)) or not (isinstance(inlier_dist, numbers.Real) or
                                                    _shape_of_values(inlier_dist, "inlier_dist") in ((), (P,))):
        raise ValueError(f"inlier_dist must be a number or ({P},) values, got {inlier_dist!r}")
    sd = _shape(depth, "depth")
    if len(sd) not in (2, 3) or 0 in sd:
        raise ValueError(f"depth must be one (dH, dW) image or (n_images, dH, dW), got shape {sd}")
    n_images, dH, dW = (1,) + sd if len(sd) == 2 else sd
    if dH * dW >= 2 ** 31:
        raise ValueError("depth frames must hold fewer than 2^31 samples")
    is_u16 = depth.dtype == (getattr(torch, "uint16", None) if isinstance(depth, torch.Tensor) else np.uint16)
    is_float = depth.dtype.is_floating_point if isinstance(depth, torch.Tensor) else np.issubdtype(depth.dtype, np.floating)
    if is_u16:
        if depth_scale is None:
            raise ValueError("uint16 depth is raw: depth_scale (millimetres per unit) is required")
        try:
            sc = np.asarray(depth_scale, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"depth_scale must be a number or one per image, got {depth_scale!r}") from None
        if sc.shape not in ((), (n_images,)) or not np.all(np.isfinite(sc)) or not np.all(sc > 0):
            raise ValueError(f"depth_scale must be a positive number or one per image, got {depth_scale!r}")
    elif not is_float:
        raise ValueError(f"depth must be uint16 (raw, with depth_scale) or floating point, got {depth.dtype}")
    elif depth_scale is not None:
        raise ValueError("float depth carries its unit already (depth_unit): depth_scale must be None")
    if depth_unit not in DEPTH_UNITS:
        raise ValueError(f"depth_unit must be one of {sorted(DEPTH_UNITS)}, got {depth_unit!r}")
    if image_index is not None and _shape_of_values(image_index, "image_index") != (P,):
        raise ValueError(f"image_index must be ({P},), got shape {_shape_of_values(image_index, 'image_index')}")
    if isinstance(iterations, bool) or not isinstance(iterations, numbers.Integral) or iterations <= 0:
        raise ValueError(f"iterations must be a positive integer, got {iterations!r}")
    return P, H, W, st[1], n_images, dH, dW


def depth_on_device(depth, dev, depth_scale=None, depth_unit="m"):
    """depth (dH, dW) or (n_images, dH, dW) -> (n_images, dH, dW) float32 on `dev` in the unit of the network's 3-D points (metres).
    Floating point: used as it is (depth_unit "m") or scaled from millimetres (depth_unit "mm").  uint16: raw values with
    `depth_scale` (millimetres per unit, a number or one per image), converted by pp_depth_u16_scaled: (f32(d) * f32(scale)) / 1000."""
    is_t = isinstance(depth, torch.Tensor)
    if depth.ndim == 2:
        depth = depth[None]
    if depth_scale is None:
        d = depth if is_t else torch.from_numpy(np.ascontiguousarray(depth))
        d = d.to(device=dev, dtype=torch.float32).contiguous()
        return d if depth_unit == "m" else d * DEPTH_UNITS[depth_unit]
    return depth_u16_scaled(depth, np.broadcast_to(np.asarray(depth_scale, dtype=np.float64), (len(depth),)).astype(np.float32), dev)


def rgbd_launch(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, depth, inlier_dist, image_index=None, iterations=150,
                return_inliers=False, depth_scale=None, depth_unit="m"):
    """Enqueue the batched kernel on the current stream; returns DEVICE tensors without synchronising: rot (P,3,3) f64, tvec (P,3)
    f64, ratio (P) f64, ok, npts, nlisted (P) i32, rms (P) f64 [, mask (P,N) uint8 with return_inliers].  Arguments as
    pose_recovery_ransac_rgbd_batched."""
    P, H, W, N, n_images, dH, dW = check_rgbd_args(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, depth, inlier_dist,
                                                   image_index, iterations, depth_scale, depth_unit)
    t2, s3, Kd, pose = _lib.dev_f32(tar_pts_2d, src_pts_3d, K, tem_pose)
    tp, sp = tar_pts.contiguous().long(), src_pts.contiguous().long()
    dev = t2.device
    dep = depth_on_device(depth, dev, depth_scale, depth_unit)
    if isinstance(inlier_dist, numbers.Real):
        dist = torch.full((P,), float(inlier_dist), dtype=torch.float32, device=dev)
    else:
        dist = torch.as_tensor(inlier_dist).to(device=dev, dtype=torch.float32).expand(P).contiguous()
    if image_index is None:
        img = torch.zeros(P, dtype=torch.int32, device=dev)
    else:
        img = torch.as_tensor(image_index).to(device=dev, dtype=torch.int32).contiguous()
    rot, tvec, ratio, ok, npts = alloc_pose_outputs(P, dev)
    nlisted = torch.empty(P, dtype=torch.int32, device=dev)
    rms = torch.empty(P, dtype=torch.float64, device=dev)
    mask = torch.empty(P, N, dtype=torch.uint8, device=dev) if return_inliers else None
    _lib.call("pp_rgbd_ransac", t2, s3, Kd, pose, tp, sp, P, H, W, N, dep, n_images, dH, dW, img, dist, int(iterations),
              rot, tvec, ratio, ok, npts, nlisted, rms, mask)
    return (rot, tvec, ratio, ok, npts, nlisted, rms) + ((mask,) if return_inliers else ())


def _packed(launched):
    """The launch's results as ONE (P, 17) f64 device tensor."""
    rot, tvec, ratio, ok, npts, nlisted, rms = launched[:7]
    P = rot.shape[0]
    return torch.cat([rot.reshape(P, 9), tvec, ratio[:, None], ok.double()[:, None], npts.double()[:, None], nlisted.double()[:, None],
                      rms[:, None]], dim=1)


def _unpacked(host, P):
    """host (P, 17) -> rot, tvec, ratio, ok, npts, stats."""
    return (host[:, :9].reshape(P, 3, 3).copy(), host[:, 9:12].reshape(P, 3, 1).copy(), host[:, 12].copy(), host[:, 13] != 0,
            host[:, 14].astype("int32"), dict(num_listed=host[:, 15].astype("int32"), rms=host[:, 16].copy()))


def pose_recovery_ransac_rgbd_batched(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, depth, inlier_dist, image_index=None,
                                      iterations=150, return_inliers=False, *, depth_scale=None, depth_unit="m"):
    """All (instance, hypothesis) problems of a batch in ONE launch and ONE device->host copy; mirrors
    utils.pose_recovery.pose_recovery_ransac_pnp_batched, whose first six arguments these are:
    tar_pts_2d (P,2,H,W), src_pts_3d (P,3,H,W), K (P,3,3), tem_pose (P,4,4), tar_pts / src_pts (P,N,2) int64 with -1 padding, N <= 4096.

    depth: the test depth image(s), (dH, dW) or (n_images, dH, dW), numpy or tensor.  Floating point in the unit of src_pts_3d
    (the network's: metres; depth_unit="mm" for float millimetres, scaled on the device), or uint16 raw values with depth_scale
    (millimetres per unit, a number or one per image; converted to metres on the device).  A value that is not finite or not > 0
    is missing.  image_index (P,): the image each problem reads (default 0).
    inlier_dist: the inlier radius, a DISTANCE in the unit of src_pts_3d: a number or (P,) values.  It has no default: it
    depends on the object's size and the sensor's noise — choose it as a fraction of the object's diameter.
    iterations: RANSAC hypotheses per problem (at most 256 are run).

    -> rot (P,3,3) f64, tvec (P,3,1) f64, inliers_ratio (P) f64, success (P) bool, npts (P) int32 (pairs with a depth),
    stats = dict(num_listed (P) int32: entries of the lists without -1, rms (P) f64: RMS 3-D residual of the consensus set)
    (numpy arrays) [+ inliers (P,N) bool in the order of the listed entries, with return_inliers].  A failed problem returns
    (I, [0,0,1]^T, 0.0, False) like the PnP.  ValueError, before any device work, for malformed arguments (check_rgbd_args)."""
    launched = rgbd_launch(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, depth, inlier_dist, image_index, iterations,
                           return_inliers, depth_scale, depth_unit)
    P = launched[0].shape[0]
    res = _unpacked(_packed(launched).cpu().numpy(), P)
    return res + (launched[7].cpu().numpy() != 0,) if return_inliers else res


class RgbdHandle:
    """A batched RGB-D launch whose result is on its way to the host (pose_recovery_ransac_rgbd_batched_async)."""
    __slots__ = ("host", "event", "P", "mask")

    def __init__(self, host, event, P, mask=None):
        self.host, self.event, self.P, self.mask = host, event, P, mask

    def result(self):
        """Wait for the copy and unpack, as pose_recovery_ransac_rgbd_batched returns it."""
        self.event.synchronize()
        res = _unpacked(self.host.numpy(), self.P)
        return res + (self.mask.numpy() != 0,) if self.mask is not None else res


def pose_recovery_ransac_rgbd_batched_async(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, depth, inlier_dist, image_index=None,
                                            iterations=150, return_inliers=False, *, depth_scale=None, depth_unit="m", host=None,
                                            stream=None):
    """pose_recovery_ransac_rgbd_batched without the host wait: the launch and ONE asynchronous device->host copy (P x 17 doubles
    into a pinned buffer, `host` to reuse one) are enqueued; `.result()` of the returned handle waits for them.
    stream: a side torch.cuda.Stream for the launch and the copy (it first waits for the current stream, i.e. for the forward that
    produced the inputs).  This solver reads no operand the forward could have clamped beyond what the PnP reads, so it carries no
    saturation slot: that verdict belongs to the forward and travels with the PnP's copy."""
    check_rgbd_args(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, depth, inlier_dist, image_index, iterations, depth_scale,
                    depth_unit)
    inputs = (tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts)
    on_device = [t for t in inputs + (depth, inlier_dist, image_index) if isinstance(t, torch.Tensor) and t.is_cuda]
    host, ev, P, mask = launch_and_copy_async(
        lambda: rgbd_launch(*inputs, depth, inlier_dist, image_index, iterations, return_inliers, depth_scale, depth_unit),
        _packed, stream, on_device, host, 7 if return_inliers else None)
    return RgbdHandle(host, ev, P, mask=mask)


def pose_recovery_ransac_rgbd(tar_pts_2d, src_pts_3d, K, tem_pose, tar_pts, src_pts, depth, inlier_dist, iterations=150,
                              return_inliers=False, *, depth_scale=None, depth_unit="m"):
    """One problem (one instance / hypothesis), like utils.pose_recovery.pose_recovery_ransac_pnp: tar_pts_2d (2,H,W),
    src_pts_3d (3,H,W), K (3,3), tem_pose (4,4), tar_pts / src_pts (N,2), depth one (dH, dW) image, inlier_dist a number
    -> (rot ndarray(3,3), tvec ndarray(3,1), inliers_ratio float, success bool, npts int, stats dict(num_listed, rms))
    [+ inliers (N,) bool].  It is batch index 0 of the batched call: a problem's sampling depends on its index."""
    for name, x, nd in (("tar_pts_2d", tar_pts_2d, 3), ("src_pts_3d", src_pts_3d, 3), ("K", K, 2), ("tem_pose", tem_pose, 2),
                        ("tar_pts", tar_pts, 2), ("src_pts", src_pts, 2), ("depth", depth, 2)):
        if len(_shape(x, name)) != nd:
            raise ValueError(f"{name} must have {nd} dimensions for one problem, got shape {_shape(x, name)}")
    res = pose_recovery_ransac_rgbd_batched(tar_pts_2d[None], src_pts_3d[None], K[None], tem_pose[None], tar_pts[None], src_pts[None],
                                            depth, inlier_dist, None, iterations, return_inliers, depth_scale=depth_scale,
                                            depth_unit=depth_unit)
    rot, tvec, ratio, ok, npts, st = res[:6]
    out = (rot[0], tvec[0], float(ratio[0]), bool(ok[0]), int(npts[0]), dict(num_listed=int(st["num_listed"][0]), rms=float(st["rms"][0])))
    return out + (res[6][0],) if return_inliers else out
