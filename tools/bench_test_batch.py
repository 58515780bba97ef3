"""Test-image assembly (picopose_amd/provider/test_batch.py) against the per-detection loop it replaces, in one process.

(a) the loop: numpy decode of each RLE to a frame-sized mask + utils.preprocess.crop_instance per detection + collation by
hand; (b) assemble_test_image.  For 8 and 32 detections on 480x640 and 960x1280 frames: host wall clock of the call (no
synchronise inside the window; one after it, outside), HIP events around the call, median and p10-p90 over --iters calls
after warm-up, and the bytes each leg copies host -> device.  --latency: pipeline.infer_image per image with (a) and (b)
in front, at the reference's regime (8 detections, chunks of 4; ViT-L, 162 templates).  --profile: a short loop of (b) then
(a) for a rocprofv3 kernel trace.  Prints JSON lines.
usage: bench_test_batch.py [--iters 50] [--latency] [--profile]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detections_oracle as do  # noqa: E402

from picopose_amd.provider import test_batch as tb  # noqa: E402
from picopose_amd.utils import preprocess as hp  # noqa: E402


def make_image(seed, H, W, n):
    """A textured frame and n detections as CNOS writes them (compressed RLE): elliptic blobs of 1/8 - 1/2 of the frame, a
    tenth of them with 10 % holes."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    dets = [do.record(do.blob(rng, H, W, holes=0.1 if j % 10 == 9 else 0.0), 0.9 - 0.01 * j, 1 + j % 2, time=0.1) for j in range(n)]
    K = [572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0]
    return img, dets, K, {1: 0, 2: 1}


def loop_by_hand(img, dets, K, obj_idxs, device="cuda"):
    """Leg (a): what a user writes around crop_instance today."""
    kept = [d for d in dets if d["score"] > 0.0]
    rows = [hp.crop_instance(img, do.decode(d["segmentation"]), d["bbox"], device=device) for d in kept]
    n = len(rows)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(device)  # noqa: E731
    i32 = lambda a: torch.from_numpy(np.asarray(a, np.int32)).to(device)  # noqa: E731
    return {"score": f32([[d["score"]] for d in kept])[None], "obj_id": i32([[d["category_id"]] for d in kept])[None],
            "obj_idx": i32([[obj_idxs[d["category_id"]]] for d in kept])[None],
            "real_pts2d": torch.stack([r["pts2d"].float() for r in rows]).to(device)[None],
            "real_rgb": torch.stack([r["rgb"] for r in rows])[None], "real_bbox": f32([r["bbox"] for r in rows])[None],
            "real_mask": torch.stack([r["mask"] for r in rows])[None], "real_M": torch.stack([r["M"] for r in rows]).to(device)[None],
            "real_K": f32(np.array(K, np.float64).reshape(3, 3))[None].repeat(n, 1, 1)[None],
            "real_pose": torch.eye(4, device=device)[None].repeat(n, 1, 1)[None],
            "scene_id": i32([[1]]), "img_id": i32([[7]]), "seg_time": f32([[dets[0]["time"]]])}


def measure(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    host, ev = [], []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e3)
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    q = lambda v: [float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90))]  # noqa: E731
    return {"host_ms_median_p10_p90": q(host), "event_ms_median_p10_p90": q(ev)}


def h2d_bytes(img, dets, n):
    H, W = img.shape[:2]
    runs = sum(len(tb.rle_counts(d["segmentation"])) for d in dets)
    small = 4 * (runs + (n + 1) + 4 * n + 2 * n + 2 + n + n * 64 * 64 * 2 + 4 * n + 9 * n + 9 * n + 16 * n + 1)
    by_hand = n * (H * W * 3 + H * W) + 4 * (n + 2 * n + 2 + n * 64 * 64 * 2 + 4 * n + 9 * n + 9 + 1)
    return {"assemble": H * W * 3 + small, "loop": by_hand, "run_ends": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--latency", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    cases = [(H, W, n) for (H, W) in ((480, 640), (960, 1280)) for n in (8, 32)]
    if a.profile:
        for H, W, n in cases:
            args = make_image(100 + n, H, W, n)
            for _ in range(8):
                tb.assemble_test_image(*args, scene_id=1, img_id=7)
            for _ in range(3):
                loop_by_hand(*args)
        torch.cuda.synchronize()
        return
    for H, W, n in cases:
        args = make_image(100 + n, H, W, n)
        x, y = tb.assemble_test_image(*args, scene_id=1, img_id=7), loop_by_hand(*args)
        same = all(torch.equal(x[k], y[k]) for k in y)
        # alternate the legs so that both see the same box conditions
        res = {"loop": [], "assemble": []}
        for _ in range(2):
            res["loop"].append(measure(lambda: loop_by_hand(*args), a.iters // 2))
            res["assemble"].append(measure(lambda: tb.assemble_test_image(*args, scene_id=1, img_id=7), a.iters // 2))
        print(json.dumps({"what": "test_image_assembly", "frame": [H, W], "detections": n, "outputs_identical": same,
                          "h2d_bytes": h2d_bytes(args[0], args[1], n), "loop_crop_instance": res["loop"],
                          "assemble_test_image": res["assemble"]}), flush=True)
    if a.latency:
        import bench
        from picopose_amd.picopose import Net
        from picopose_amd.pipeline import infer_image

        vit, N, n_obj, hyp, bs, n_det = "dinov2_vitl14", 162, 2, 5, 4, 8
        net = Net(bench.make_cfg(vit))
        bench.seeded_weights(net, 4, vit)
        net = net.cuda().eval()
        net.match_mode = "fast"
        tem = bench.make_end_points(n_obj, N, "cuda", 300)
        templates = {k: v for k, v in tem.items() if k.startswith("tem_")}
        with torch.no_grad():
            templates["template_feature"] = torch.stack([torch.cat([net.feature_extractor(tem["tem_rgb"][o, s:s + bs])[-1]
                                                                    for s in range(0, N, bs)]) for o in range(n_obj)])
        images = [make_image(500 + i, 480, 640, n_det) for i in range(8)]
        out = {}
        from picopose_amd import ops

        ops.SATURATION_FLAG = False        # random crops through calibrated random weights: the walk is what is timed
        for name, front in (("loop_crop_instance", loop_by_hand), ("assemble_test_image", lambda *p: tb.assemble_test_image(*p, scene_id=1, img_id=7))):
            ms = []
            for i, im in enumerate(images):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.no_grad():
                    preds = infer_image(net, front(*im), templates, hyp=hyp, bs=bs)
                ms.append((time.perf_counter() - t0) * 1e3)
                assert len(preds) == n_det
            out[name + "_ms_per_image_median"] = float(np.median(ms[2:]))
            out[name + "_ms_per_image_all"] = [round(v, 2) for v in ms]
        print(json.dumps({"what": "infer_image per image incl. preprocessing (ViT-L, 162 templates, 8 detections, chunks of 4)", **out}),
              flush=True)


if __name__ == "__main__":
    main()
