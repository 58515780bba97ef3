"""Proposal labelling (picopose_amd/proposals.py, csrc/pp_proposals.hip): the numbers of profiles/r07/proposals.md, one process.

match:    one pp_proposal_match call (both launches) at P = 200 queries, 30 objects x 42 views, C = 1024, next to
          torch.matmul + topk + mean + max on the same unit rows, the two legs alternating; HIP events around bursts of calls.
overlaps: pp_rle_pack_bits + pp_mask_intersections for 100 elliptic masks of a 480 x 640 frame (tables already on the device),
          and mask_overlaps from the records (host decode and upload included).
call:     label_proposals for 200 proposals of a 480 x 640 frame on the ViT of the benchmark's default workload (ViT-B/14, seeded
          weights) against a bank of 30 x 42 random unit rows: whole call, and its sections with a synchronise after each.
Prints JSON lines.  usage: bench_proposals.py [--iters 7] [--burst 20]"""
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

from picopose_amd import _lib, masks  # noqa: E402
from picopose_amd import proposals as pr  # noqa: E402


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def burst_ms(fn, burst):
    """Milliseconds per call: HIP events around `burst` calls enqueued back to back."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(burst):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / burst


def bench_match(iters, burst, P=200, O=30, V=42, C=1024, topk=5):
    g = torch.Generator().manual_seed(1)
    bank = pr.DescriptorBank.from_rows(torch.randn(O * V, C, generator=g).cuda(), [V] * O, list(range(O)))
    q = pr.normalize_descriptors(torch.randn(P, C, generator=g).cuda())
    score, view = torch.empty((P, O), device="cuda"), torch.empty((P, O), dtype=torch.int32, device="cuda")
    label, best = torch.empty((P,), dtype=torch.int32, device="cuda"), torch.empty((P,), device="cuda")

    def hip():
        _lib.call("pp_proposal_match", q, P, bank.rows, bank.offsets, bank.offsets_host, O, C, topk, score, view, label, best)

    def torch_leg():
        cos = torch.matmul(q, bank.rows.t()).view(P, O, V)
        s = cos.topk(topk, dim=2).values.mean(2)
        return s, cos.argmax(2), s.max(1)

    hip()
    s_t, v_t, (b_t, l_t) = torch_leg()
    torch.cuda.synchronize()
    agree = {"max_abs_score_diff": float((s_t - score).abs().max()), "labels_equal": bool((l_t.int() == label).all()),
             "views_equal": bool((v_t.int() == view).all())}
    for _ in range(3):
        burst_ms(hip, burst), burst_ms(torch_leg, burst)
    t_hip, t_torch = [], []
    for _ in range(iters):
        t_hip.append(burst_ms(hip, burst))
        t_torch.append(burst_ms(torch_leg, burst))
    print(json.dumps({"what": "match", "P": P, "objects": O, "views": V, "C": C, "topk": topk, "burst": burst, "iters": iters,
                      "pp_proposal_match_ms": stats(t_hip), "torch_matmul_topk_mean_max_ms": stats(t_torch), "agreement": agree,
                      "flop": 2 * P * O * V * C, "bank_bytes": 4 * O * V * C}), flush=True)


def bench_overlaps(iters, burst, n=100, H=480, W=640):
    rng = np.random.default_rng(2)
    recs = [do.record(do.blob(rng, H, W, holes=0.1 if j % 10 == 9 else 0.0), 0.5, 1) for j in range(n)]
    segs = [r["segmentation"] for r in recs]
    table = masks.RunTable.upload([masks.run_ends(masks.rle_counts(s)) for s in segs], "cuda")
    pack = lambda: table.pack(H * W)  # noqa: E731  (the launch and its two output allocations, as every caller has it)
    bits, _ = pack()
    words, n_runs = bits.shape[1], table.n_runs
    inter = torch.empty((n, n), dtype=torch.int32, device="cuda")
    sect = lambda: _lib.call("pp_mask_intersections", bits, n, words, inter)  # noqa: E731
    for _ in range(3):
        burst_ms(pack, burst), burst_ms(sect, burst)
    t_pack, t_sect, t_call = [], [], []
    for _ in range(iters):
        t_pack.append(burst_ms(pack, burst))
        t_sect.append(burst_ms(sect, burst))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, b = pr.mask_overlaps(segs, (H, W))
        b.cpu()
        t_call.append((time.perf_counter() - t0) * 1e3)
    dense = np.stack([do.decode(s).ravel(order="F") for s in segs]).astype(np.int64)
    print(json.dumps({"what": "overlaps", "masks": n, "frame": [H, W], "words": words, "run_ends": n_runs, "burst": burst, "iters": iters,
                      "pp_rle_pack_bits_ms": stats(t_pack), "pp_mask_intersections_ms": stats(t_sect),
                      "mask_overlaps_call_ms": stats(t_call), "equals_dense_numpy": bool(np.array_equal(inter.cpu().numpy(), dense @ dense.T))}),
          flush=True)


def bench_call(iters, n=200, H=480, W=640, O=30, V=42, vit="dinov2_vitb14"):
    import bench
    from picopose_amd.picopose import Net

    C = bench.VIT[vit][0]
    net = Net(bench.make_cfg(vit))
    bench.seeded_weights(net, 4, vit)
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(3)
    bank = pr.DescriptorBank.from_rows(torch.randn(O * V, C, generator=g).cuda(), [V] * O, list(range(1, O + 1)))
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    props = [{"segmentation": do.record(do.blob(rng, H, W), 0.5, 1)["segmentation"]} for _ in range(n)]
    kw = dict(scene_id=1, img_id=1, min_score=-1.0)               # random weights: every proposal passes the cut, 100 reach the NMS
    for _ in range(2):
        out = pr.label_proposals(net, img, props, bank, **kw)
    whole, parts = [], []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pr.label_proposals(net, img, props, bank, **kw)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
        t = {}
        pr.label_proposals(net, img, props, bank, timings=t, **kw)
        parts.append({k: v * 1e3 for k, v in t.items()})
    print(json.dumps({"what": "label_proposals", "proposals": n, "frame": [H, W], "vit": vit, "objects": O, "views": V, "bs": 16,
                      "records": len(out), "iters": iters, "whole_call_ms": stats(whole),
                      "sections_ms": {k: stats([p[k] for p in parts]) for k in parts[0]}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--burst", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    bench_match(a.iters, a.burst)
    bench_overlaps(a.iters, a.burst)
    bench_call(a.iters)


if __name__ == "__main__":
    main()
