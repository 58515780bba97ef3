"""Writes tests/golden/warmup_cosine_lr.json: the learning rates of the reference's WarmupCosineLR (utils/lr_scheduler.py:306-356),
run on CPU over a torch.optim.SGD, for several argument sets at iterations 0, 1, 999, 1000, 1001, a few in the middle and max_iters.

    python tools/gen_warmup_cosine_golden.py --reference <path of the reference checkout>

Only the lr values are stored (no code of the reference); tests/test_optim_cpu.py checks picopose_amd.optim.WarmupCosineLR against them."""
import argparse
import importlib.util
import json
import os
import warnings

import torch

CASES = [
    dict(max_iters=400000, warmup_factor=0.001, warmup_iters=1000),                       # run_train.py:88 with config/base.yaml
    dict(max_iters=400000, warmup_factor=0.001, warmup_iters=1000, warmup_method="constant"),
    dict(max_iters=400000, warmup_factor=0.001, warmup_iters=1000, start_cos_after_warmup=True),
    dict(max_iters=400000, warmup_factor=0.01, warmup_iters=1000, cycle_factor=0.5),
    dict(max_iters=5000, warmup_factor=0.1, warmup_iters=0),
    dict(max_iters=5000, warmup_factor=0.001, warmup_iters=1000, cycle_factor=2.0),
]
BASE_LRS = [1e-5, 3e-4]       # two param groups


def iterations(max_iters):
    its = [0, 1, 999, 1000, 1001, max_iters // 4, max_iters // 2 - 1, max_iters // 2, 3 * max_iters // 4, max_iters]
    return sorted(set(i for i in its if 0 <= i <= max_iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds utils/lr_scheduler.py)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden",
                                                  "warmup_cosine_lr.json"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_lr_scheduler", os.path.join(a.reference, "utils", "lr_scheduler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {"base_lrs": BASE_LRS, "cases": []}
    for args in CASES:
        params = [torch.nn.Parameter(torch.zeros(1)) for _ in BASE_LRS]
        opt = torch.optim.SGD([{"params": [p], "lr": lr} for p, lr in zip(params, BASE_LRS)], lr=BASE_LRS[0])
        sched = mod.WarmupCosineLR(opt, **args)
        want = set(iterations(args["max_iters"]))
        lrs = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")        # (scheduler stepped without optimizer steps)
            for it in range(args["max_iters"] + 1):
                if it in want:
                    lrs[str(it)] = [g["lr"] for g in opt.param_groups]
                if it < args["max_iters"]:
                    sched.step()
        out["cases"].append({"args": args, "lr": lrs})
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(a.out)


if __name__ == "__main__":
    main()
