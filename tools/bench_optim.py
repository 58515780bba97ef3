"""Times the reference's optimizer step at the ViT-B trained parameter set (GPU; no reference code needed).

    python tools/bench_optim.py [--pairs 32] [--steps 5] [--iters 20]

1. optimizer.step() + the next forward's re-split of the trained linears (ops.split_weight_dev on every parameter the engine keeps a
   device-scaled operand of), torch.optim.AdamW(foreach=True) against picopose_amd.optim.AdamW (whose step writes those operands
   itself); per-pass times of ours (pass 1 alone = the step with the engine in f32, which has no operands to split) and the achieved
   bandwidth as a fraction of 6.3 TB/s.
2. The full training step of bench.py's train leg (forward_train under autograd + Loss + backward + optimizer step) with each optimizer."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402
from picopose_amd import ops  # noqa: E402
from picopose_amd.optim import AdamW  # noqa: E402
from picopose_amd.picopose import Net  # noqa: E402
from picopose_amd.utils.loss_utils import Loss  # noqa: E402
from picopose_amd.utils.seeding import calibrated_state_dict  # noqa: E402

PEAK = 6.3e12
KW = dict(lr=1e-5, betas=(0.5, 0.999), eps=1e-6, weight_decay=5e-4)   # config/base.yaml:9-14


def make_net(vit, pairs):
    from netcfg import make_train_end_points

    net = Net(bench.make_cfg(vit))
    net.load_state_dict(calibrated_state_dict(net.state_dict(), 4, vit))
    net = net.cuda().train()
    ep = {k: v.cuda() for k, v in make_train_end_points(pairs, 11).items()}
    return net, ep


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def step_bench(net, ep, iters, out):
    Loss()(net(dict(ep)))["loss"].backward()
    trained = [p for p in net.parameters() if p.grad is not None]
    targets, _ = ops.device_split_targets(trained)
    split_ps = [trained[i] for i, _, _ in targets]
    n_all = sum(p.numel() for p in trained)
    n_split = sum(p.numel() for p in split_ps)
    out(f"trained tensors {len(trained)}, elements {n_all / 1e6:.1f} M; split in the step: {len(split_ps)} tensors, {n_split / 1e6:.1f} M")
    snapshot = [p.detach().clone() for p in trained]

    def restore():
        with torch.no_grad():
            for p, s in zip(trained, snapshot):
                p.copy_(s)

    ref = torch.optim.AdamW(trained, foreach=True, **KW)

    def torch_step():
        ref.step()
        for p in split_ps:
            ops.split_weight_dev(p)

    t_torch = timed(torch_step, iters)
    del ref
    restore()
    torch.cuda.empty_cache()
    ours = AdamW(trained, **KW)
    t_ours = timed(ours.step, iters)
    old = ops.PRECISION
    ops.PRECISION = "f32"
    try:
        t_pass1 = timed(ours.step, iters)
    finally:
        ops.PRECISION = old
    ours.step()          # (rebuild the table with the split targets again)
    t_pass2 = t_ours - t_pass1
    b1, b2 = 28.0 * n_all, 8.0 * n_split
    out(f"torch AdamW(foreach) step + re-split of the {len(split_ps)} operands: {t_torch:.3f} ms")
    out(f"picopose_amd AdamW step (pass 1 + pass 2):                  {t_ours:.3f} ms  ({t_torch / t_ours:.2f}x)")
    out(f"  pass 1 (update, {b1 / 1e9:.2f} GB): {t_pass1:.3f} ms = {b1 / t_pass1 / 1e9:.2f} TB/s = {b1 / t_pass1 * 1e3 / PEAK:.2f} of 6.3 TB/s"
        " (incl. the host-side step and the record upload)")
    out(f"  pass 2 (split, {b2 / 1e9:.2f} GB): {t_pass2:.3f} ms = {b2 / max(t_pass2, 1e-6) / 1e9:.2f} TB/s = "
        f"{b2 / max(t_pass2, 1e-6) * 1e3 / PEAK:.2f} of 6.3 TB/s (difference of the two timings)")
    del ours
    restore()
    net.zero_grad(set_to_none=True)
    torch.cuda.empty_cache()


def train_bench(vit, pairs, steps, make_opt, out, label):
    net, ep = make_net(vit, pairs)
    opt, times = None, []
    for i in range(steps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Loss()(net(dict(ep)))["loss"].backward()
        if opt is None:
            opt = make_opt([p for p in net.parameters() if p.grad is not None])
        opt.step()
        opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        if i >= 2:
            times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    out(f"full training step ({vit}, {pairs} pairs, f16x3) with {label}: median {times[len(times) // 2]:.1f} ms, min {times[0]:.1f} ms "
        f"over {len(times)} steps")
    del net, opt
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vit", default="dinov2_vitb14")
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    out = lambda s: print(s, flush=True)  # noqa: E731
    ops.PRECISION = "f16x3"
    out(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    net, ep = make_net(a.vit, a.pairs)
    step_bench(net, ep, a.iters, out)
    del net, ep
    torch.cuda.empty_cache()
    if not a.no_train:
        train_bench(a.vit, a.pairs, a.steps, lambda ps: torch.optim.AdamW(ps, foreach=True, **KW), out, "torch.optim.AdamW(foreach)")
        train_bench(a.vit, a.pairs, a.steps, lambda ps: AdamW(ps, **KW), out, "picopose_amd.optim.AdamW")
        train_bench(a.vit, a.pairs, a.steps, lambda ps: torch.optim.SGD(ps, lr=1e-6), out, "torch.optim.SGD (bench.py's train leg)")


if __name__ == "__main__":
    main()
