"""Training-pair assembly (picopose_amd/provider/training_batch.py) at B pairs of 640 x 480 frames with the reference's settings
(augment_real, p 0.8; templates not augmented; rgb_mask_flag off; size_ratio 1).

Prints JSON lines: the assembly's GPU time (HIP events around the whole enqueue, median over --iters after warm-up) and that of
its H2D copies alone, the host time of the call, bytes moved per executor pass, the numpy/PIL oracle pipeline per pair on
--workers CPU processes (a stand-in for a CPU loader: imgaug is not available), and with --step the training step (ViT-B,
forward_train + Loss + backward) with and without the assembly in front.  --profile: a short loop for a rocprofv3 kernel trace.
usage: bench_train_batch.py [--batch 32] [--iters 50] [--workers 16] [--step] [--profile]"""
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

from picopose_amd.provider import training_batch as tb  # noqa: E402

H, W = 480, 640


def make_pair(seed):
    """A decoded pair like a MegaPose frame: textured 640 x 480 image, an object blob of 60-260 px, uint16 depth; a template of
    the same size with an alpha blob."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.clip(128 + 60 * np.sin(yy / rng.uniform(5, 40))[..., None] + rng.normal(0, 20, (H, W, 3)), 0, 255).astype(np.uint8)
    s = int(rng.integers(60, 260))
    y, x = int(rng.integers(0, H - s)), int(rng.integers(0, W - s))
    mask = np.zeros((H, W), np.uint8)
    mask[y:y + s, x:x + s] = (yy[:s, :s] - s / 2) ** 2 + (xx[:s, :s] - s / 2) ** 2 < (s / 2) ** 2
    rgba = np.zeros((H, W, 4), np.uint8)
    rgba[..., :3] = rgb[::-1]
    a = int(rng.integers(100, 300))
    rgba[240 - a // 2:240 + a // 2, 320 - a // 2:320 + a // 2, 3] = 255
    pose = np.eye(4)
    pose[:3, 3] = (0, 0, 8000)
    return {"rgb": rgb, "mask": mask, "depth": rng.integers(500, 3000, (H, W), dtype=np.uint16), "depth_scale": 0.1,
            "K": np.array([[572.4, 0, 320], [0, 573.6, 240], [0, 0, 1]]), "cam_R_m2c": np.eye(3).ravel(), "cam_t_m2c": [0, 0, 700],
            "tem_rgba": rgba, "tem_depth": rng.integers(500, 3000, (H, W), dtype=np.uint16), "tem_pose": pose}


def _oracle_pair(args):
    import train_batch_oracle as ob

    seed, n = args
    pairs = [make_pair(seed + k) for k in range(n)]
    progs = tb.ColorAugmentor(np.random.default_rng(seed)).sample(n)
    t = time.perf_counter()
    ob.collate(pairs, progs, [tb.EMPTY] * n)
    return time.perf_counter() - t


def events_ms(fn, iters):
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    B = a.batch
    samples = [make_pair(1000 + k) for k in range(B)]
    gen = np.random.default_rng(0)
    run = lambda: tb.assemble_training_batch(samples, generator=gen)  # noqa: E731
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    if a.profile:
        for _ in range(10):
            run()
        torch.cuda.synchronize()
        return
    t = events_ms(run, a.iters)
    host = []
    for _ in range(10):
        t0 = time.perf_counter()
        run()
        host.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    # the H2D copies alone: the same pinned buffers the call fills (frames with the mask byte, depths)
    hbuf = [torch.empty((B, H, W, 3), dtype=torch.uint8, pin_memory=True), torch.empty((B, H, W), dtype=torch.uint8, pin_memory=True),
            torch.empty((B, H, W, 4), dtype=torch.uint8, pin_memory=True)] + \
           [torch.empty((B, H, W), dtype=torch.int16, pin_memory=True) for _ in range(2)]
    h2d = events_ms(lambda: [x.to("cuda", non_blocking=True) for x in hbuf], a.iters)
    print(json.dumps({"what": "assemble_training_batch", "B": B, "frame": [H, W], "gpu_ms_median": float(np.median(t)),
                      "gpu_ms_p10_p90": [float(np.percentile(t, 10)), float(np.percentile(t, 90))],
                      "h2d_ms_median": float(np.median(h2d)), "h2d_bytes": int(sum(x.numel() * x.element_size() for x in hbuf)),
                      "host_call_ms_median": float(np.median(host))}), flush=True)

    # bytes per executor pass (one read + one write of 4-byte pixels per crop pixel; neighbour reads hit the caches), the
    # resize (crop read, 3 fp32 planes + mask written) and the depth conversions (2 bytes in, 4 out)
    progs = tb.ColorAugmentor(np.random.default_rng(0)).sample(B)
    boxes = [tb._prepare(s, 1.0, 1.0, 224)["bbox"] for s in samples]
    crops = [(0, 0, W, bx, 0) for bx in boxes] + [(1, 0, W, tb._prepare(s, 1.0, 1.0, 224)["tem_bbox"], 1) for s in samples]
    plan = tb.plan_augmentation(crops, list(progs) + [tb.EMPTY] * B)
    hw = plan.desc[:, 5].astype(np.int64) * plan.desc[:, 6]
    per_pass = [int(8 * hw[plan.desc[:, 10] > p].sum()) for p in range(tb.MAX_PASSES)]
    print(json.dumps({"what": "executor_bytes_per_pass", "bytes": per_pass, "crop_pixels": int(hw.sum()),
                      "resize_bytes": int(4 * hw.sum() + 2 * B * 224 * 224 * 16), "depth_bytes": int(2 * B * H * W * 6)}), flush=True)

    from multiprocessing import get_context

    n_per = 4
    with get_context("spawn").Pool(a.workers) as pool:
        pool.map(_oracle_pair, [(1, 1)] * a.workers)                 # worker start-up and imports outside the timing
        t0 = time.perf_counter()
        secs = pool.map(_oracle_pair, [(2000 + 10 * k, n_per) for k in range(a.workers * 2)])
        wall = time.perf_counter() - t0
    pairs = a.workers * 2 * n_per
    print(json.dumps({"what": "numpy_oracle_pipeline (stand-in for a CPU loader; imgaug absent)", "workers": a.workers,
                      "s_per_pair_one_process_median": float(np.median(secs)) / n_per,
                      "pairs_per_s_all_workers_wall": pairs / wall}), flush=True)

    if a.step:
        from netcfg import make_train_end_points
        import types

        from picopose_amd.picopose import Net
        from picopose_amd.utils.loss_utils import Loss
        from picopose_amd.utils.seeding import calibrated_state_dict

        ns = types.SimpleNamespace
        vit = "dinov2_vitb14"
        cfg = ns(hypothesis=5, stage1=ns(vit_type=vit, pretrained=False, interaction_indexes=[[0, 2], [3, 5], [6, 8], [9, 11]]),
                 stage2=ns(in_channel=256, hidden_dim=256),
                 stage3=ns(nclass=1, in_channels=768, use_bn=True, out_channels=[256, 512, 1024, 1024], num_levels=3, radius=4))
        net = Net(cfg)
        net.load_state_dict(calibrated_state_dict(net.state_dict(), 4, vit))
        net = net.cuda().train()
        fixed = {k: v.cuda() for k, v in make_train_end_points(B, 11).items()}

        def step(ep):
            net.zero_grad(set_to_none=True)
            Loss()(net(ep))["loss"].backward()

        res = {}
        for name, fn in (("step_fixed_batch", lambda: step(fixed)), ("step_with_assembly", lambda: step(run()))):
            for _ in range(2):
                fn()
            res[name + "_ms_median"] = float(np.median(events_ms(fn, 8)))
        print(json.dumps({"what": "train_step_vitb", "B": B, **res}), flush=True)


if __name__ == "__main__":
    main()
