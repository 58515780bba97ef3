"""Cost of the batched RGB-D pose recovery (pp_rgbd_ransac) next to the RGB-only PnP (pp_pnp_ransac) on the same correspondence lists.

The bench's PnP regime: --problems 160 x --points 3500 correspondences, 150 iterations, 30 % outliers (and 20 problems with
--problems 20).  The lists are those of tests/rgbd_pose_oracle.make_problem, so the planted pose explains the pixels (for the PnP)
and the depth (for the RGB-D solver) at once.  Both C entries are called directly on preallocated outputs; a sample is the time
between two HIP events around --burst back-to-back launches of one solver, divided by the burst (a single RGB-D launch is shorter
than its enqueue), after a warm-up, the two solvers alternated, median of --runs.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rgbd_pose_oracle as ro  # noqa: E402

from picopose_amd import _lib  # noqa: E402
from picopose_amd.rgbd_pose import rgbd_launch  # noqa: E402
from picopose_amd.utils.pose_recovery import pnp_launch  # noqa: E402

KEYS = ("tar2d", "src3d", "K", "pose", "tar_pts", "src_pts")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, nargs="+", default=[160, 20])
    ap.add_argument("--points", type=int, default=3500)
    ap.add_argument("--outliers", type=float, default=0.3)
    ap.add_argument("--noise", type=float, default=0.001)
    ap.add_argument("--inlier-dist", type=float, default=0.005)
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures the MI355X"
    res = {"points": a.points, "iterations": a.iterations, "outliers": a.outliers, "runs": a.runs, "burst": a.burst}
    for P in a.problems:
        # 480 x 640 frames: 307 200 pixels each, enough distinct pixels for 160 x 3500 pairs over two images
        scene = ro.Scene(np.random.default_rng(0), n_images=2, dH=480, dW=640)
        probs = [ro.make_problem(scene, a.points, a.outliers, a.noise, image=i % 2, inlier_dist=a.inlier_dist) for i in range(P)]
        args = [torch.from_numpy(np.stack([p[k] for p in probs])).cuda() for k in KEYS]
        depth = torch.from_numpy(scene.depth).cuda()
        dist = torch.full((P,), a.inlier_dist, dtype=torch.float32, device="cuda")
        img = torch.tensor([p["image"] for p in probs], dtype=torch.int32, device="cuda")
        L, st = _lib.lib(), _lib.stream_ptr()
        H, W, N = args[0].shape[2], args[0].shape[3], args[4].shape[1]
        ptr = [t.data_ptr() for t in args]
        out = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device="cuda")  # noqa: E731
        o_rot, o_t, o_ratio, o_rms = out(P, 9), out(P, 3), out(P), out(P)
        o_ok, o_n, o_nl = (out(P, dtype=torch.int32) for _ in range(3))

        def pnp():
            _lib.check(L.pp_pnp_ransac(*ptr, P, H, W, N, a.iterations, 2.0, o_rot.data_ptr(), o_t.data_ptr(), o_ratio.data_ptr(),
                                       o_ok.data_ptr(), o_n.data_ptr(), st), "pp_pnp_ransac")

        def rgbd():
            _lib.check(L.pp_rgbd_ransac(*ptr, P, H, W, N, depth.data_ptr(), depth.shape[0], depth.shape[1], depth.shape[2], img.data_ptr(),
                                        dist.data_ptr(), a.iterations, o_rot.data_ptr(), o_t.data_ptr(), o_ratio.data_ptr(), o_ok.data_ptr(),
                                        o_n.data_ptr(), o_nl.data_ptr(), o_rms.data_ptr(), None, st), "pp_rgbd_ransac")

        forms = {"pnp": pnp, "rgbd": rgbd}
        for _ in range(a.warmup):
            for f in forms.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(a.runs):
            for name, f in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.burst):
                    f()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.burst)
        ok_pnp = pnp_launch(*args, a.iterations)[3]
        ratio, ok_rgbd = rgbd_launch(*args, depth, dist, img, a.iterations)[2:4]
        for name, ts in times.items():
            res[f"{name}_ms_median_P{P}"] = float(np.median(ts))
            res[f"{name}_ms_min_P{P}"] = float(np.min(ts))
            res[f"{name}_ms_max_P{P}"] = float(np.max(ts))
        res[f"success_P{P}"] = {"pnp": int(ok_pnp.sum().item()), "rgbd": int(ok_rgbd.sum().item())}
        res[f"rgbd_ratio_mean_P{P}"] = float(ratio.mean().item())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
