"""Cost and effect of the Levenberg-Marquardt tail of the batched PnP (refine="lm", pp_pnp_ransac_refine).

Times the PnP launch alone, with and without refinement, at the headline shape (160 problems x ~3 500 correspondences, 30 %
outliers, 0.5 px): HIP events around each launch, warm-up first, the two forms alternated, median of --runs.  Then the accuracy
ratio of tests/test_pnp_refine_gpu.py (200 problems, 3 500 points, 30 % outliers, 1 px): median rotation / translation error
against the planted pose, refined over unrefined.  Prints one JSON line (and writes it to --out).
--profile: only launches (--runs of each form, no timing), for `rocprofv3 --kernel-trace --stats -- python tools/bench_pnp_refine.py
--profile`, which gives the kernel durations of both instantiations."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pnp_problems import make_batch, pose_errors  # noqa: E402

from picopose_amd.utils.pose_recovery import pnp_launch, pose_recovery_ransac_pnp_batched  # noqa: E402

KEYS = ("tar2d", "src3d", "K", "pose", "tar_pts", "src_pts")


def _args(b):
    return [torch.from_numpy(b[k]).cuda() for k in KEYS]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=160)
    ap.add_argument("--points", type=int, default=3500)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures the MI355X"
    args = _args(make_batch(np.random.default_rng(0), a.problems, a.points, 0.3, 0.5))
    forms = {"plain": {}, "lm": dict(refine="lm")}
    if a.profile:
        for _ in range(a.runs):
            for kw in forms.values():
                pnp_launch(*args, **kw)
        torch.cuda.synchronize()
        print(json.dumps({"profile_launches_per_form": a.runs}))
        return
    for _ in range(a.warmup):
        for kw in forms.values():
            pnp_launch(*args, **kw)
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.runs):
        for name, kw in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pnp_launch(*args, **kw)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    res = {"problems": a.problems, "points": a.points, "runs": a.runs}
    for name, ts in times.items():
        res[f"{name}_ms_median"] = float(np.median(ts))
        res[f"{name}_ms_min"] = float(np.min(ts))
        res[f"{name}_ms_max"] = float(np.max(ts))
    res["added_ms_median"] = res["lm_ms_median"] - res["plain_ms_median"]
    st = pose_recovery_ransac_pnp_batched(*args, refine="lm")[4]
    res["lm_iterations_mean"] = float(st["iterations"].mean())
    res["lm_iterations_max"] = int(st["iterations"].max())
    # accuracy against the planted pose (the regime of tests/test_pnp_refine_gpu.py::test_refinement_improves_the_median_pose_error)
    b = make_batch(np.random.default_rng(60), 200, 3500, 0.3, 1.0)
    rot0, tvec0 = pose_recovery_ransac_pnp_batched(*_args(b))[:2]
    rot1, tvec1 = pose_recovery_ransac_pnp_batched(*_args(b), refine="lm")[:2]
    a0, t0 = pose_errors(rot0, tvec0, b["R"], b["t"])
    a1, t1 = pose_errors(rot1, tvec1, b["R"], b["t"])
    res.update(rot_err_deg_median_plain=float(np.median(a0)), rot_err_deg_median_lm=float(np.median(a1)),
               trans_err_rel_median_plain=float(np.median(t0)), trans_err_rel_median_lm=float(np.median(t1)),
               rot_err_ratio=float(np.median(a1) / np.median(a0)), trans_err_ratio=float(np.median(t1) / np.median(t0)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
