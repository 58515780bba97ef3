"""Depth proposals (csrc/pp_depth_proposals.hip, picopose_amd/depth_proposals.py) on one GPU: what each stage costs at 480 x 640.
The frame is an analytic tilted table (tests/depth_proposals_oracle.table_scene) with twelve raised boxes and 10 % invalid pixels; B = 1,
8, 32 copies with different seeds of the invalid pixels.

  * per stage wrapper (HIP events around a burst of calls; the wrapper allocates its outputs, nothing waits for the device):
    plane_fit at n_hyp 256 and 1024, components, component_stats, component_rle (its two launches and the host read between them);
  * the whole depth_proposals call (host clock around the call, which ends with the proposals on the host);
  * the yardstick of the other profile rows in the same process: scene_gt.scene_gt_info for 8 views of a 20 480-face mesh.

Every row: median, min and max over the repeats after the warm-up.  One JSON line per row.  `--abi-only` runs only the stage wrappers
of one batch size, for a rocprofv3 kernel trace (tile / border / flatten and the other kernels by name).  Numbers:
profiles/r16/depth_proposals.md."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_proposals_oracle as do  # noqa: E402  (scene builder only)
import render_oracle as ro  # noqa: E402  (mesh generator only)

from picopose_amd import depth_proposals as dp  # noqa: E402

H, W = 480, 640
RECTS = tuple((40 + 150 * r, 130 + 150 * r, 30 + 155 * c, 140 + 155 * c, 50.0 + 10 * (r * 4 + c)) for r in range(3) for c in range(4))


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def events(fn, reps, warmup, burst):
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


def wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def batch(B):
    frames = [do.table_scene(H, W, RECTS, invalid=0.1, seed=s, keep_rects=True) for s in range(B)]
    cam = frames[0][1]
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], np.float64)
    return np.stack([f[0] for f in frames]), np.stack([cam] * B), K


def stages(B, a):
    depth_h, cams_h, K = batch(B)
    depth, cams = torch.from_numpy(depth_h).cuda(), torch.from_numpy(cams_h).cuda()
    row = lambda what, ms, **kw: print(json.dumps({"what": what, "images": B, "ms": stats(ms), **kw}), flush=True)  # noqa: E731
    for n_hyp in (256, 1024):
        row("plane_fit", events(lambda: dp.plane_fit(depth, cams, n_hyp=n_hyp), a.reps, a.warmup, a.burst), n_hyp=n_hyp)
    fit = dp.plane_fit(depth, cams)
    has = fit["info"][:, 0].contiguous()
    ms = events(lambda: dp.components(depth, cams, fit["plane"], has), a.reps, a.warmup, a.burst)
    row("components", ms, bytes_per_call=8 * B * H * W, gbytes_per_s=round(8 * B * H * W / statistics.median(ms) / 1e6, 1))
    labels = dp.components(depth, cams, fit["plane"], has)
    row("component_stats", events(lambda: dp.component_stats(labels, min_area=200, max_area=H * W // 2), a.reps, a.warmup, a.burst))
    n_q, recs = (t.cpu().numpy() for t in dp.component_stats(labels, min_area=200, max_area=H * W // 2))
    sel = np.concatenate([np.concatenate([np.full((n_q[b], 1), b, np.int32), recs[b, :n_q[b]][:, [0, 2, 3, 4, 5]]], axis=1) for b in range(B)])
    row("component_rle", events(lambda: dp.component_rle(labels, sel), a.reps, a.warmup, a.burst), components=len(sel))
    if not a.abi_only:
        row("depth_proposals", wall(lambda: dp.depth_proposals(depth_h, K), a.reps, a.warmup), proposals=int(n_q.sum()),
            info=fit["info"][0].tolist())


def yardstick(a):
    from picopose_amd import evaluation as ev
    from picopose_amd import scene_gt as sg

    m = ro.icosphere(5, 50.0)
    models = ev.ObjectModels({1: {"vertices": m["vertices"], "faces": m["faces"], "info": {"diameter": 100.0}}})
    U = 8
    rng = np.random.default_rng(0)
    t = np.stack([rng.uniform(-250, 250, U), rng.uniform(-180, 180, U), rng.uniform(620, 640, U)], axis=1).astype(np.float32)
    R = np.tile(np.eye(3, dtype=np.float32), (U, 1, 1))
    K = np.array([[600.0, 0, (W - 1) / 2], [0, 600.0, (H - 1) / 2], [0, 0, 1]])
    depth = np.full((1, H, W), 630.0, dtype=np.float32)
    fn = lambda: sg.scene_gt_info(models, np.ones(U, dtype=np.int64), R, t, K, depth=depth)  # noqa: E731
    print(json.dumps({"what": "scene_gt_info", "views": U, "ms": stats(events(fn, a.reps, a.warmup, 1))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--abi-only", action="store_true", help="only the stage wrappers (for a rocprofv3 kernel trace)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--burst", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_proposals needs the GPU: a timing taken elsewhere says nothing")
    print(json.dumps({"what": "setup", "frame": [H, W], "boxes": len(RECTS), "device": torch.cuda.get_device_name(0)}), flush=True)
    if not a.abi_only:
        yardstick(a)
    for B in a.images:
        stages(B, a)
    if not a.abi_only:
        yardstick(a)


if __name__ == "__main__":
    main()
