"""Pose verification (`pp_pose_verify`, picopose_amd/verify.py) on one GPU: what a call costs next to the raster it is built on.
640 x 480 frame, f = 600, one icosphere of radius 50 mm with 20 480 faces, U = 8 / 40 / 160 views spread over the frame at Z = 620 .. 640 mm (the setup of profiles/r07/scene_gt.md); one 96 x 96 box mask per view around its
projected centre; the test depth is flat at 630 mm, so views in front of it agree or are seen through and views behind it are hidden.

  * per Python call (HIP events around the call, host planning and uploads included): evaluation.render_depth — the yardstick —
    and verify.verify_poses with and without the depth image;
  * per ABI call on one packed scene (tables, masks and depth already on the device; HIP events around a burst of calls):
    pp_pose_verify with and without depth, ALTERNATING burst by burst, for window "auto" (the raster dominates) and window "full"
    (307 200 samples per view: the reduction dominates).  This is the row in which a variant of the reduction kernel is compared:
    profiles/r15/pose_verify.md holds the comparison of the two mask walks, taken with this loop on a build that had both.

Every row: median, min and max over the repeats after the warm-up.  One JSON line per row.  Numbers: profiles/r15/pose_verify.md."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_oracle as ro  # noqa: E402  (mesh generator only)

from picopose_amd import _lib  # noqa: E402
from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import masks  # noqa: E402
from picopose_amd import scene as scn  # noqa: E402
from picopose_amd import scene_gt as sg  # noqa: E402
from picopose_amd import verify as vf  # noqa: E402

H, W, FOCAL = 480, 640, 600.0
K = np.array([[FOCAL, 0, (W - 1) / 2], [0, FOCAL, (H - 1) / 2], [0, 0, 1]], dtype=np.float64)


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def events(fn, reps, warmup, burst=1):
    """Milliseconds per call of fn: HIP events around `burst` calls, `reps` times after `warmup` bursts."""
    for _ in range(warmup * burst):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / burst)
    return out


def views(U):
    rng = np.random.default_rng(0)
    t = np.stack([rng.uniform(-250, 250, U), rng.uniform(-180, 180, U), rng.uniform(620, 640, U)], axis=1).astype(np.float32)
    R = np.tile(np.eye(3, dtype=np.float32), (U, 1, 1))
    segs = []
    for x, y, z in t:
        u, v = int(round(FOCAL * x / z + K[0, 2])), int(round(FOCAL * y / z + K[1, 2]))
        m = np.zeros((H, W), dtype=bool)
        m[max(v - 48, 0):v + 48, max(u - 48, 0):u + 48] = True
        segs.append(sg.rle_from_mask(m))
    return R, t, segs


def python_calls(models, U, a):
    R, t, segs = views(U)
    ids = np.ones(U, dtype=np.int64)
    depth = np.full((1, H, W), 630.0, dtype=np.float32)
    rows = {"render_depth": lambda: ev.render_depth(models, ids, R, t, K, (H, W)),
            "verify_poses_depth": lambda: vf.verify_poses(models, ids, R, t, K, segs, (H, W), depth=depth),
            "verify_poses_rgb": lambda: vf.verify_poses(models, ids, R, t, K, segs, (H, W))}
    for name, fn in rows.items():
        print(json.dumps({"what": "python_call", "call": name, "views": U, "ms": stats(events(fn, a.reps, a.warmup))}), flush=True)
    r = vf.verify_poses(models, ids, R, t, K, segs, (H, W), depth=depth)
    c = r["counts"].sum(dim=0).tolist()
    print(json.dumps({"what": "counts", "views": U, "sum": dict(zip(vf.COUNTS, c)), "mean_score": round(float(r["score"].mean()), 4)}), flush=True)


def abi_calls(models, U, window, a):
    """One packed scene; the calls with and without depth alternate burst by burst so that drift hits both alike."""
    R, t, segs = views(U)
    dev = models.device
    obj, img = np.zeros(U, dtype=np.int32), np.zeros(U, dtype=np.int32)
    cams = scn.cameras(K, 1)
    poses = scn.pose44(R, t)
    windows = scn.view_windows(models, obj, img, poses, cams, H, W, 1.0, window)
    packed = scn.PackedScene(models, cams, H, W, 1.0, obj, img, poses, windows)
    L, need = _lib.lib(), ctypes.c_size_t()
    _lib.check(L.pp_vsd_workspace_bytes(packed.samples, packed.faces, ctypes.byref(need)), "pp_vsd_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    bits, _ = masks.RunTable.upload([masks.run_ends(masks.rle_counts(s, size=(H, W))) for s in segs], dev).pack(H * W)
    words, i32p = bits.shape[1], ctypes.POINTER(ctypes.c_int)
    vm = np.arange(U, dtype=np.int32)
    vm_d = torch.from_numpy(vm).to(dev)
    depth = torch.full((1, H, W), 630.0, dtype=torch.float32, device=dev)
    counts = torch.empty((U, 8), dtype=torch.int32, device=dev)
    near = torch.empty((U,), dtype=torch.int32, device=dev)

    def call(with_depth):
        _lib.check(L.pp_pose_verify(ctypes.byref(packed.scene), bits.data_ptr(), U, words, vm_d.data_ptr(), vm.ctypes.data_as(i32p),
                                    depth.data_ptr() if with_depth else None, 15.0, ws.data_ptr(), ws.numel(), counts.data_ptr(),
                                    near.data_ptr(), _lib.stream_ptr()), "pp_pose_verify")

    ms = {True: [], False: []}
    for d in ms:
        events(lambda: call(d), 0, a.warmup, a.burst)
    for _ in range(a.reps):
        for d in ms:
            ms[d] += events(lambda: call(d), 1, 0, a.burst)
    print(json.dumps({"what": "abi_call", "views": U, "window": window, "window_samples": packed.samples, "burst": a.burst,
                      "depth_ms": stats(ms[True]), "rgb_ms": stats(ms[False])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="*", default=[8, 40, 160])
    ap.add_argument("--full-views", type=int, nargs="*", default=[8, 40], help="view counts of the window='full' rows")
    ap.add_argument("--abi-only", action="store_true", help="skip the Python-call rows (for a rocprofv3 kernel trace of the ABI rows)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--burst", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_verify needs the GPU: a timing taken elsewhere says nothing")
    m = ro.icosphere(5, 50.0)
    models = ev.ObjectModels({1: {"vertices": m["vertices"], "faces": m["faces"], "info": {"diameter": 100.0}}})
    print(json.dumps({"what": "setup", "frame": [H, W], "faces": int(len(m["faces"])), "device": torch.cuda.get_device_name(0)}), flush=True)
    for U in ([] if a.abi_only else a.views):
        python_calls(models, U, a)
    for U in a.views:
        abi_calls(models, U, "auto", a)
    for U in a.full_views:
        abi_calls(models, U, "full", a)


if __name__ == "__main__":
    main()
