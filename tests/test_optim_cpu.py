"""picopose_amd.optim without a GPU: the WarmupCosineLR sequence against the reference's (tests/golden/warmup_cosine_lr.json, written by
tools/gen_warmup_cosine_golden.py), argument validation of pp_adam_multi_tensor, and the optimizers' constructor rejections."""
import ctypes
import json
import os
import warnings

import pytest
import torch

from picopose_amd import _lib
from picopose_amd.optim import Adam, AdamW, WarmupCosineLR, build_optimizer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warmup_cosine_lr.json")


def test_warmup_cosine_lr_matches_the_reference_sequence():
    gold = json.load(open(GOLDEN))
    base = gold["base_lrs"]
    assert len(gold["cases"]) >= 5
    for case in gold["cases"]:
        args = case["args"]
        params = [torch.nn.Parameter(torch.zeros(1)) for _ in base]
        opt = torch.optim.SGD([{"params": [p], "lr": lr} for p, lr in zip(params, base)], lr=base[0])
        sched = WarmupCosineLR(opt, **args)
        seen = 0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            it = 0
            while True:
                want = case["lr"].get(str(it))
                if want is not None:
                    got = [g["lr"] for g in opt.param_groups]
                    for w, g in zip(want, got):
                        assert abs(g - w) <= 1e-12 * abs(w), (args, it, g, w)
                    assert sched.get_last_lr() == got
                    seen += 1
                if it >= args["max_iters"]:
                    break
                if it > 1100:      # (past the warm-up every step is checked at the fixture's points only: jump to the next one)
                    nxt = min(int(k) for k in case["lr"] if int(k) > it)
                    sched.last_epoch = nxt - 1
                opt.step()
                sched.step()
                it = sched.last_epoch
        assert seen == len(case["lr"])


def test_warmup_cosine_lr_rejects_an_unknown_warmup_method():
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    with pytest.raises(ValueError):
        WarmupCosineLR(opt, max_iters=10, warmup_iters=5, warmup_method="exp")


def test_adam_multi_tensor_argument_validation():
    L = _lib.lib()
    T = _lib.PpAdamTensor
    p = ctypes.c_void_p(256)
    need = ctypes.c_size_t()
    good = (T * 1)(T(256, 512, 768, None, None, 1024))
    assert L.pp_adam_workspace_bytes(good, 1, ctypes.byref(need)) == 0 and need.value >= 256   # host-side sizing only
    assert L.pp_adam_workspace_bytes(None, 1, ctypes.byref(need)) == -1
    assert L.pp_adam_workspace_bytes(good, 0, ctypes.byref(need)) == -1                     # tensor count <= 0
    assert L.pp_adam_workspace_bytes(good, 1, None) == -1
    for bad in (T(None, 512, 768, None, None, 1024), T(256, None, 768, None, None, 1024), T(256, 512, None, None, None, 1024),
                T(256, 512, 768, None, None, 0), T(256, 512, 768, None, None, -8),
                T(256, 512, 768, 1024, None, 1024),          # a split target without its scale pair
                T(256, 512, 768, 1024, 2048, 1020),          # split target with n % 8 != 0
                T(260, 512, 768, 1024, 2048, 1024)):         # split target whose parameter is not 16-byte aligned
        arr = (T * 1)(bad)
        assert L.pp_adam_workspace_bytes(arr, 1, ctypes.byref(need)) == -1
        assert L.pp_adam_multi_tensor(arr, 1, p, 2, 1, p, 1 << 20, None) == -1
    assert L.pp_adam_multi_tensor(None, 1, p, 2, 1, p, 1 << 20, None) == -1
    assert L.pp_adam_multi_tensor(good, 0, p, 2, 1, p, 1 << 20, None) == -1
    assert L.pp_adam_multi_tensor(good, -1, p, 2, 1, p, 1 << 20, None) == -1
    assert L.pp_adam_multi_tensor(good, 1, None, 2, 1, p, 1 << 20, None) == -1               # no step records
    assert L.pp_adam_multi_tensor(good, 1, p, 2, 1, None, 1 << 20, None) == -1               # no workspace
    assert L.pp_adam_multi_tensor(good, 1, p, 3, 1, p, 1 << 20, None) == -1                  # terms
    assert L.pp_adam_multi_tensor(good, 1, p, 2, 1, p, 16, None) == -2                       # workspace too small: PP_EWORKSPACE


@pytest.mark.parametrize("cls", [AdamW, Adam])
def test_constructor_rejections(cls):
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ValueError, match="amsgrad"):
        cls([p], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        cls([p], maximize=True)
    with pytest.raises(TypeError, match="float32"):
        cls([torch.nn.Parameter(torch.zeros(8, dtype=torch.float64))])
    with pytest.raises(ValueError, match="contiguous"):
        cls([torch.nn.Parameter(torch.zeros(8, 4).t())])
    with pytest.raises(ValueError, match="GPU"):          # a CPU parameter: the step is a HIP kernel, no fallback
        cls([p])
    with pytest.raises(ValueError, match="learning rate"):
        cls([p], lr=-1.0)
    with pytest.raises(ValueError, match="beta"):
        cls([p], betas=(1.0, 0.999))


def test_build_optimizer_types():
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ValueError, match="SGD"):
        build_optimizer({"type": "SGD", "lr": 1e-5, "betas": [0.5, 0.999], "eps": 1e-6, "weight_decay": 5e-4}, [p])
    with pytest.raises(ValueError, match="GPU"):          # the AdamW branch is taken (and refuses the CPU parameter)
        build_optimizer({"type": "AdamW", "lr": 1e-5, "betas": [0.5, 0.999], "eps": 1e-6, "weight_decay": 5e-4}, [p])


def test_param_group_keys_are_torchs():
    ours = set(AdamW.__init__.__code__.co_varnames[:AdamW.__init__.__code__.co_argcount + AdamW.__init__.__code__.co_kwonlyargcount])
    theirs = set(torch.optim.AdamW.__init__.__code__.co_varnames[:torch.optim.AdamW.__init__.__code__.co_argcount
                                                                    + torch.optim.AdamW.__init__.__code__.co_kwonlyargcount])
    assert ours == theirs
    import inspect
    for cls, ref in ((AdamW, torch.optim.AdamW), (Adam, torch.optim.Adam)):
        a, b = inspect.signature(cls.__init__).parameters, inspect.signature(ref.__init__).parameters
        assert list(a) == list(b) or set(a) == set(b)
        for k in a:
            if k != "params" and k != "self":
                assert a[k].default == b[k].default, (cls, k)
