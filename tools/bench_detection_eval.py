"""Timings of detection scoring (picopose_amd/detection_eval.py) on the card: the pp_rle_pack_bits, pp_det_overlaps and pp_det_match
launches (device events), the whole score_detections call (host clock; the call ends with downloads, so it has waited for the device),
next to the numpy restatement on the host (tests/detection_eval_oracle.py, literal loops) and next to the route the library offered
before: proposals.mask_overlaps over the union of an image's masks, image by image (all pairs of the image, no matching).

    python tools/bench_detection_eval.py [--images 1 64 1000] [--repeats 5] [--oracle-images 1] [--out FILE.json]

Per image: 640 x 480, 100 detections and 15 ground truths over 10 categories, rectangles written directly as run lengths (a detection is
a shifted ground truth of its category or clutter).  Every shape is warmed up once; the figures are the median and the minimum of
`repeats` runs.  No GPU: an error, never a CPU figure."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, N_DET, N_GT, N_CAT = 480, 640, 100, 15, 10


def rect_rle(y0, y1, x0, x1):
    """The uncompressed COCO run lengths of the rectangle rows [y0, y1), columns [x0, x1) in an H x W frame."""
    h, n = y1 - y0, x1 - x0
    counts = np.empty(2 * n + 1, np.int64)
    counts[0] = x0 * H + y0
    counts[1::2] = h
    counts[2::2] = H - h
    counts[-1] = H * W - (x1 - 1) * H - y1
    return {"size": [H, W], "counts": counts.tolist()}


def make(n_images, seed=0):
    rng = np.random.default_rng(seed)
    dets, anns = [], []
    for im in range(n_images):
        boxes = []
        for j in range(N_GT):
            h, w = int(rng.integers(20, 200)), int(rng.integers(20, 200))
            y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
            boxes.append((j % N_CAT + 1, y, x, h, w))
            anns.append({"scene_id": 1, "image_id": im, "category_id": j % N_CAT + 1, "bbox": [x, y, w, h], "segmentation": rect_rle(y, y + h, x, x + w),
                         "ignore": False, "iscrowd": False})
        for i in range(N_DET):
            if i < 3 * N_GT:                                                # near a ground truth of the category
                c, y, x, h, w = boxes[i % N_GT]
                y, x = int(np.clip(y + rng.integers(-8, 9), 0, H - h)), int(np.clip(x + rng.integers(-8, 9), 0, W - w))
            else:
                c, h, w = i % N_CAT + 1, int(rng.integers(10, 120)), int(rng.integers(10, 120))
                y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
            dets.append({"scene_id": 1, "image_id": im, "category_id": c, "bbox": [x, y, w, h], "score": float(rng.random()), "time": 0.0,
                         "segmentation": rect_rle(y, y + h, x, x + w)})
    return dets, anns


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "runs": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[1, 64, 1000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--oracle-images", type=int, default=1, help="the largest case the literal-loop restatement is timed on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_detection_eval needs the GPU")
    import detection_eval_oracle as eo

    from picopose_amd import detection_eval as de
    from picopose_amd import proposals

    rows = []
    for n in args.images:
        dets, anns = make(n)
        row = {"images": n, "detections": len(dets), "annotations": len(anns)}
        for iou_type in ("segm", "bbox"):
            de.score_detections(dets, anns, iou_type=iou_type)                  # warm-up of this shape
            whole, parts = [], {"pack": [], "overlaps": [], "match": []}
            for _ in range(args.repeats if n < 1000 else 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s = de.score_detections(dets, anns, iou_type=iou_type)
                whole.append(time.perf_counter() - t0)
                tm = {}
                m = de.match_detections(dets, anns, iou_type=iou_type, timings=tm)
                for k in parts:
                    parts[k].append(tm.get(k, 0.0))
            row[iou_type] = {"score_detections": stats(whole), "AP": s["AP"], "pairs": int(len(m["iou"])), "chunks": m["n_chunks"],
                             **{k: stats(v) for k, v in parts.items() if iou_type == "segm" or k != "pack"}}
        # the earlier route to the same intersections: all pairs of an image's masks, image by image (decode, upload, pack, intersect, download)
        per = {}
        for r in dets + anns:
            per.setdefault(r["image_id"], []).append(r["segmentation"])
        proposals.mask_overlaps(per[0], (H, W))[0].cpu()
        old = []
        for _ in range(args.repeats if n < 1000 else 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for segs in per.values():
                inter, area = proposals.mask_overlaps(segs, (H, W))
                inter.cpu(), area.cpu()
            old.append(time.perf_counter() - t0)
        row["mask_overlaps_per_image"] = stats(old)
        if n <= args.oracle_images:
            t0 = time.perf_counter()
            ref = eo.score(dets, anns)
            row["oracle_segm"] = {"ms": 1e3 * (time.perf_counter() - t0), "AP": ref["AP"]}
            t0 = time.perf_counter()
            eo.score(dets, anns, iou_type="bbox")
            row["oracle_bbox"] = {"ms": 1e3 * (time.perf_counter() - t0)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
