"""Timings of 6D detection scoring (picopose_amd/pose_detection_eval.py) on the card: the evaluation.pose_errors call, the
pp_pose_match launch and the pp_pose_nms launch (device events), the whole score_pose_detections and pose_nms calls (host clock; both
end with downloads, so they have waited for the device), next to the same matching done by the literal host loops of the numpy
restatement (tests/pose_detection_oracle.py) in the same process, on the errors the device produced.

    python tools/bench_pose_detection.py [--images 10 100 1000] [--repeats 3] [--oracle-images 1000] [--out FILE.json]

Per image 10 objects; per (image, object) 0 .. 10 estimates and 0 .. 5 instances (uniform), so about 5 x 2.5 pairs per group.  The
models are 10 point sets of 20 480 vertices, object 1 with the cube's 24 rotations as symmetries, the others with none.  An estimate is
a ground-truth pose moved by 0.02 .. 0.6 diameters, a copy of an earlier estimate of its group (a duplicate for the suppression) or
clutter.  Every shape is warmed up once; the figures are the median and the minimum of `repeats` runs.  No GPU: an error, never a CPU
figure."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_OBJ, N_VERT, MAX_EST, MAX_GT = 10, 20480, 10, 5
K = np.array([[600.0, 0, 320], [0, 600, 240], [0, 0, 1]])


def make_models(rng):
    import pose_error_oracle as peo

    objects = {}
    for o in range(1, N_OBJ + 1):
        v = (rng.uniform(-1, 1, (N_VERT, 3)) * 60).astype(np.float32)
        info = {"diameter": 120.0 * math.sqrt(3.0)}
        if o == 1:
            info["symmetries_discrete"] = peo.cube_symmetries()
        objects[o] = {"vertices": v, "info": info}
    return objects


def make(n_images, rng):
    import pose_error_oracle as peo

    diam = 120.0 * math.sqrt(3.0)
    gt, info, cams = {1: {}}, {1: {}}, {1: {}}
    cols = {k: [] for k in ("scene_id", "im_id", "obj_id", "score", "R", "t")}
    for im in range(n_images):
        ids, Rs, ts = [], [], []
        for o in range(1, N_OBJ + 1):
            G, E = int(rng.integers(0, MAX_GT + 1)), int(rng.integers(0, MAX_EST + 1))
            Rg = [peo.random_rotation(rng) for _ in range(G)]
            tg = [np.array([rng.uniform(-400, 400), rng.uniform(-300, 300), rng.uniform(700, 1500)]) for _ in range(G)]
            ids += [o] * G
            Rs += Rg
            ts += tg
            mine = []
            for e in range(E):
                u = rng.random()
                if e < G:                                                        # near a ground truth
                    d = rng.normal(size=3)
                    pose = (Rg[e], tg[e] + d / np.linalg.norm(d) * diam * rng.uniform(0.02, 0.6))
                elif mine and u < 0.5:                                           # a duplicate of an earlier estimate
                    pose = mine[int(rng.integers(0, len(mine)))]
                else:                                                            # clutter
                    pose = (peo.random_rotation(rng), np.array([rng.uniform(-400, 400), rng.uniform(-300, 300), rng.uniform(700, 1500)]))
                mine.append(pose)
                for k, v in zip(cols, (1, im, o, float(rng.random()), pose[0], pose[1])):
                    cols[k].append(v)
        gt[1][im] = {"obj_id": np.array(ids, np.int64), "R": np.array(Rs).reshape(-1, 3, 3), "t": np.array(ts).reshape(-1, 3)}
        info[1][im] = [{"visib_fract": float(rng.random())} for _ in ids]
        cams[1][im] = {"K": K, "depth_scale": 1.0}
    est = {"scene_id": np.array(cols["scene_id"], np.int64), "im_id": np.array(cols["im_id"], np.int64), "obj_id": np.array(cols["obj_id"], np.int64),
           "score": np.array(cols["score"], np.float64), "R": np.array(cols["R"]).reshape(-1, 3, 3), "t": np.array(cols["t"]).reshape(-1, 3)}
    return est, gt, info, cams


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "runs": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--oracle-images", type=int, default=1000, help="the largest case the literal-loop restatement is timed on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_detection needs the GPU")
    import pose_detection_oracle as po

    from picopose_amd import evaluation as ev
    from picopose_amd import pose_detection_eval as pe

    rng = np.random.default_rng(0)
    models = ev.ObjectModels(make_models(rng))
    rows = []
    for n in args.images:
        est, gt, info, cams = make(n, rng)
        ann = pe.pose_annotations(gt, info)
        pe.score_pose_detections(est, ann, models, cams)                         # warm-up of this shape
        pe.pose_nms(est, models)
        whole, nms_whole, parts = [], [], {"errors": [], "match": [], "nms_errors": [], "nms": []}
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = pe.score_pose_detections(est, ann, models, cams)
            whole.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            keep = pe.pose_nms(est, models)
            nms_whole.append(time.perf_counter() - t0)
            tm = {}
            m = pe.match_poses(est, ann, models, cams, timings=tm)
            pe.pose_nms(est, models, timings=tm)
            for k in parts:
                parts[k].append(tm.get(k, 0.0))
        row = {"images": n, "estimates": len(est["score"]), "ground_truths": len(ann["obj_id"]), "ignored": int(ann["ignore"].sum()),
               "groups": len(m["group_pair"]), "pairs": int(m["n_pairs"]), "nms_pairs": int(pe.plan_nms(est)["n_tri"]), "kept_by_nms": len(keep),
               "AP": s["AP"], "AP_MSSD": s["AP_MSSD"], "AP_MSPD": s["AP_MSPD"], "score_pose_detections": stats(whole), "pose_nms": stats(nms_whole),
               **{k: stats(v) for k, v in parts.items()}}
        if n <= args.oracle_images:
            plan = {k: m[k] for k in po.LAYOUT + ("images", "objects", "n_pairs")}
            t0 = time.perf_counter()
            ref = po.match(plan, m["errors"], m["limits"])
            row["oracle_match_ms"] = 1e3 * (time.perf_counter() - t0)
            row["oracle_tables_equal"] = all(ref[k].tobytes() == m[k].tobytes() for k in po.TABLES)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
