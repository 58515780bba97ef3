"""Indexed template bank against the gathered one (profiles/r07/indexed_bank.*).

stage 1: matching_templates on bank[obj_index] (today's evaluator: one copy of the bank per crop) against
matching_templates_indexed(bank, obj_index) at B = 32, N = 162, C = 768 / 1024, fp32 / fp16 banks, FAST mode, three object
patterns: 32 distinct objects, 4 objects x 8 crops, 1 object x 32 crops; the indexed walk also at several chunk sizes (PP_S1_CPX).
Call time from HIP events, the two forms alternated over rounds (min over rounds of the mean per call).
infer_image: one synthetic image of 16 detections of 2 objects at ViT-L, N = 162, hyp 5, bs 16: ms per image and peak allocation.

--profile: every stage-1 configuration `--calls` times, nothing timed, for a rocprofv3 run (kernel trace or FETCH_SIZE); the order
of the configurations is written to --order so that the trace's s1_main dispatches can be assigned to them."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from picopose_amd.utils import matching as hm  # noqa: E402

B, N = 32, 162
PATTERNS = {"32x1": (32, lambda: torch.arange(32)), "4x8": (4, lambda: torch.arange(32) % 4), "1x32": (1, lambda: torch.zeros(32, dtype=torch.int64))}


def _inputs(C, dtype, pattern):
    O, idx_fn = PATTERNS[pattern]
    g = torch.Generator(device="cuda").manual_seed(C + O)
    bank = torch.randn(O, N, C, 16, 16, device="cuda", generator=g).to(dtype)
    idx = idx_fn().cuda()
    query = torch.randn(B, C, 16, 16, device="cuda", generator=g)
    yy, xx = torch.meshgrid(torch.arange(224.0), torch.arange(224.0), indexing="ij")
    mask = (((yy - 111.5) ** 2 + (xx - 111.5) ** 2) < (0.4 * 224) ** 2).float()[None].repeat(B, 1, 1).cuda()
    return bank, idx, query, mask


def _configs(cpx_list):
    for C in (768, 1024):
        for dtype in (torch.float32, torch.float16):
            for pattern in PATTERNS:
                yield C, dtype, pattern, [None] + ([c for c in cpx_list] if pattern != "32x1" else [])


def _call(form, bank, gathered, idx, query, mask, cpx):
    if form == "gathered":
        return hm.matching_templates(gathered, query, None, mask, topk=5, mode="fast")
    if cpx is None:
        os.environ.pop("PP_S1_CPX", None)
    else:
        os.environ["PP_S1_CPX"] = str(cpx)
    return hm.matching_templates_indexed(bank, idx, query, None, mask, topk=5, mode="fast")


def stage1(args):
    rows = []
    for C, dtype, pattern, cpxs in _configs(args.cpx):
        bank, idx, query, mask = _inputs(C, dtype, pattern)
        gathered = bank[idx]
        forms = [("gathered", None)] + [("indexed", c) for c in cpxs]
        ref = _call("gathered", bank, gathered, idx, query, mask, None)
        for form, cpx in forms:             # warm-up, and the results: identical
            got = _call(form, bank, gathered, idx, query, mask, cpx)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (C, dtype, pattern, form, cpx)
        best = {f: float("inf") for f in forms}
        for _ in range(args.rounds):
            for f in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    _call(f[0], bank, gathered, idx, query, mask, f[1])
                e1.record()
                e1.synchronize()
                best[f] = min(best[f], e0.elapsed_time(e1) / args.iters)
        os.environ.pop("PP_S1_CPX", None)
        bank_bytes = bank[0].numel() * bank.element_size()
        for (form, cpx), ms in best.items():
            row = dict(part="stage1", C=C, bank=str(dtype).split(".")[-1], pattern=pattern, form=form, cpx=cpx, ms_per_call=round(ms, 4),
                       vs_gathered=round(ms / best[("gathered", None)], 3), one_object_bank_MB=round(bank_bytes / 1e6, 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del bank, gathered
        torch.cuda.empty_cache()
    return rows


def profile(args):
    order = []
    for C, dtype, pattern, cpxs in _configs(args.cpx):
        bank, idx, query, mask = _inputs(C, dtype, pattern)
        gathered = bank[idx]
        for form, cpx in [("gathered", None)] + [("indexed", c) for c in cpxs]:
            for _ in range(args.calls):
                _call(form, bank, gathered, idx, query, mask, cpx)
            order.append(dict(C=C, bank=str(dtype).split(".")[-1], pattern=pattern, form=form, cpx=cpx, calls=args.calls))
        torch.cuda.synchronize()
        os.environ.pop("PP_S1_CPX", None)
        del bank, gathered
        torch.cuda.empty_cache()
    json.dump(order, open(args.order, "w"), indent=1)


def image(args):
    import bench
    from picopose_amd import ops
    from picopose_amd.picopose import Net
    from picopose_amd.pipeline import infer_image

    ops.SATURATION_FLAG = False         # (time and memory only; the poses are compared between the two forms below)
    vit, n_obj, n_det = "dinov2_vitl14", 2, 16
    net = Net(bench.make_cfg(vit))
    bench.seeded_weights(net, 4, vit)
    net = net.cuda().eval()
    tem = {k: v for k, v in bench.make_end_points(n_obj, N, "cuda", 11).items() if k.startswith("tem_")}
    with torch.no_grad():
        tem["template_feature"] = torch.stack([torch.cat([net.feature_extractor(tem["tem_rgb"][o][s:s + 54])[-1] for s in range(0, N, 54)])
                                               for o in range(n_obj)])
    inst = {k: v for k, v in bench.make_end_points(n_det, 1, "cuda", 12).items() if k.startswith("real_")}
    data = {k: v[None] for k, v in inst.items()}
    data["obj_idx"] = (torch.arange(n_det, device="cuda") % n_obj)[None]
    data["score"] = torch.ones(1, n_det, device="cuda")
    obj_bytes = sum(v[0].numel() * v.element_size() for v in tem.values())
    res = {}
    for indexed in (False, True, False, True):          # first pass of each: warm-up
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(args.images):
            preds = infer_image(net, data, tem, hyp=5, bs=16, indexed_bank=indexed)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.images
        res[indexed] = dict(ms_per_image=round(ms, 2), peak_alloc_MB=round((torch.cuda.max_memory_allocated() - base) / 1e6, 1), preds=preds)
    same = all(all((a["R_stage_3"] == b["R_stage_3"]).all() and (a["t_stage_3"] == b["t_stage_3"]).all() for a, b in zip(pa, pb))
               for pa, pb in zip(res[True]["preds"], res[False]["preds"]))
    rows = []
    for indexed in (False, True):
        r = dict(part="infer_image", vit=vit, N=N, detections=n_det, objects=n_obj, form="indexed" if indexed else "gathered",
                 ms_per_image=res[indexed]["ms_per_image"], peak_alloc_MB=res[indexed]["peak_alloc_MB"],
                 one_object_template_MB=round(obj_bytes / 1e6, 1), same_poses=bool(same))
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["stage1", "image", "all"], default="all")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--images", type=int, default=3)
    ap.add_argument("--cpx", type=int, nargs="*", default=[4, 8, 32])
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--order", default="s1_order.json")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    if args.profile:
        profile(args)
        sys.exit(0)
    rows = (stage1(args) if args.part in ("stage1", "all") else []) + (image(args) if args.part in ("image", "all") else [])
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
