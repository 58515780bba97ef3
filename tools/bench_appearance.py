"""The appearance score (picopose_amd/proposals.py, csrc/pp_appearance.hip): the numbers of profiles/r25/appearance.md, one process.

match: one pp_appearance_match call (both launches) at P = 100 proposals x N = 256 patches, C = 1024 and C = 768, against a bank of
       42 views, next to torch.bmm + masked max + masked mean on the same unit rows, the two legs alternating; HIP events around
       bursts of calls.
bank:  describe_templates(patches=True) for 2 objects x 42 views on the benchmark's default ViT (ViT-B/14, seeded weights): time
       and bytes, next to the cls-only bank.
call:  label_proposals for 200 proposals of a 480 x 640 frame against that bank, with and without appearance=True: whole call, and
       its sections with a synchronise after each.
Prints JSON lines.  usage: bench_appearance.py [--iters 7] [--burst 20]"""
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

from picopose_amd import _lib  # noqa: E402
from picopose_amd import proposals as pr  # noqa: E402
from bench_proposals import burst_ms, stats  # noqa: E402


def bench_match(iters, burst, C, P=100, N=256, R=42):
    g = torch.Generator().manual_seed(1)
    unit = lambda n: pr.normalize_descriptors(torch.randn(n * N, C, generator=g).cuda()).view(n, N, C)  # noqa: E731
    q, bank = unit(P), unit(R)
    q_valid = (torch.rand(P, N, generator=g) < 0.5).to(torch.uint8).cuda()
    t_valid = (torch.rand(R, N, generator=g) < 0.5).to(torch.uint8).cuda()
    rows_host = np.ascontiguousarray(np.random.default_rng(2).integers(0, R, P), dtype=np.int32)
    rows = torch.from_numpy(rows_host).cuda()
    sim, arg = torch.empty((P, N), device="cuda"), torch.empty((P, N), dtype=torch.int32, device="cuda")
    n_valid, app = torch.empty((P,), dtype=torch.int32, device="cuda"), torch.empty((P,), device="cuda")

    def hip():
        _lib.call("pp_appearance_match", q, q_valid, P, bank, t_valid, R, rows, rows_host, N, C, sim, arg, n_valid, app)

    rows_l, qv, tv = rows.long(), q_valid.bool(), t_valid.bool()

    def torch_leg():
        cos = torch.bmm(q, bank[rows_l].transpose(1, 2))                     # (P, N query, N template)
        s, a = cos.masked_fill(~tv[rows_l][:, None, :], float("-inf")).max(2)
        return s, a, (s * qv).sum(1) / qv.sum(1).clamp(min=1)

    hip()
    s_t, a_t, app_t = torch_leg()
    torch.cuda.synchronize()
    agree = {"max_abs_patch_sim_diff": float((s_t - sim).abs().max()), "max_abs_app_diff": float((app_t - app).abs().max()),
             "patch_arg_equal_share": float((a_t.int() == arg).float().mean())}
    for _ in range(3):
        burst_ms(hip, burst), burst_ms(torch_leg, burst)
    t_hip, t_torch = [], []
    for _ in range(iters):
        t_hip.append(burst_ms(hip, burst))
        t_torch.append(burst_ms(torch_leg, burst))
    flop = 2 * P * N * N * C
    print(json.dumps({"what": "match", "P": P, "N": N, "C": C, "views": R, "burst": burst, "iters": iters, "pp_appearance_match_ms": stats(t_hip),
                      "torch_bmm_masked_max_mean_ms": stats(t_torch), "agreement": agree, "flop": flop,
                      "tflops_at_median": round(flop / (float(np.median(t_hip)) * 1e-3) / 1e12, 2)}), flush=True)


def bench_bank_and_call(iters, n=200, H=480, W=640, O=2, V=42, vit="dinov2_vitb14"):
    import bench
    from picopose_amd.picopose import Net

    net = Net(bench.make_cfg(vit))
    bench.seeded_weights(net, 4, vit)
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(224.0), torch.arange(224.0), indexing="ij")
    disk = (((yy - 111.5) ** 2 + (xx - 111.5) ** 2) < (0.4 * 224) ** 2).float()
    tem = {"tem_rgb": torch.randn(O, V, 3, 224, 224, generator=g).cuda(), "tem_mask": disk[None, None].repeat(O, V, 1, 1).cuda()}
    ids = list(range(1, O + 1))
    t_plain, t_patch = [], []
    for _ in range(1 + min(iters, 3)):
        for patches, t in ((False, t_plain), (True, t_patch)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bank = pr.describe_templates(net, tem, ids, patches=patches)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"what": "bank", "vit": vit, "objects": O, "views": V, "describe_templates_ms": stats(t_plain[1:]),
                      "describe_templates_patches_ms": stats(t_patch[1:]), "cls_bytes": bank.rows.numel() * 4,
                      "patch_bytes": bank.patch_rows.numel() * 4 + bank.patch_valid.numel(),
                      "patch_bytes_per_object": (bank.patch_rows.numel() * 4 + bank.patch_valid.numel()) // O}), flush=True)
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    props = [{"segmentation": do.record(do.blob(rng, H, W), 0.5, 1)["segmentation"]} for _ in range(n)]
    for appearance in (False, True):
        kw = dict(scene_id=1, img_id=1, min_score=-1.0, max_detections=n, appearance=appearance)      # every proposal reaches the appearance term
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
        print(json.dumps({"what": "label_proposals", "appearance": appearance, "proposals": n, "frame": [H, W], "vit": vit, "objects": O,
                          "views": V, "bs": 16, "records": len(out), "iters": iters, "whole_call_ms": stats(whole),
                          "sections_ms": {k: stats([p[k] for p in parts]) for k in parts[0]}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--burst", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    for C in (1024, 768):
        bench_match(a.iters, a.burst, C)
    bench_bank_and_call(a.iters)


if __name__ == "__main__":
    main()
