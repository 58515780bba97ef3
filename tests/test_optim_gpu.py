"""GPU: the fused Adam / AdamW step (picopose_amd.optim, csrc/pp_optim.hip) against torch's optimizers, the state_dict hand-over in both
directions, the operand split written by the step (bit for bit pp_split_weights_ws, and no re-split in the next forward) and the
optimizer loop of run_train.py:109-130 on the ViT-S slice."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

gpu = pytest.mark.gpu

SIZES = [(1,), (7,), (8,), (768, 3072), (3072, 768), (10_000_003,)]
REF = dict(betas=(0.5, 0.999), eps=1e-6)            # config/base.yaml:9-14


def _tensors(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g).mul_(0.05) for s in SIZES]


def _groups(ps, wd=5e-4):
    return [{"params": ps[0::2], "weight_decay": wd}, {"params": ps[1::2], "weight_decay": 0.0}]


def _within_ulps(a, b, n=2):
    inf = torch.tensor(float("inf"), device=a.device)
    ulp = torch.maximum(torch.nextafter(a.abs(), inf) - a.abs(), torch.nextafter(b.abs(), inf) - b.abs())
    bad = (a - b).abs() > n * ulp
    if bad.any():
        print(f"{int(bad.sum())} of {a.numel()} beyond {n} ulp; worst {float(((a - b).abs() / ulp).max()):.1f} ulp")
    return not bool(bad.any())


def _pair(cls_ours, cls_torch, seed=0, lr=1e-3):
    from picopose_amd.optim import WarmupCosineLR

    init = _tensors(seed)
    pa = [torch.nn.Parameter(t.cuda()) for t in init]
    pb = [torch.nn.Parameter(t.cuda()) for t in init]
    oa = cls_ours(_groups(pa), lr=lr, **REF)
    ob = cls_torch(_groups(pb), lr=lr, foreach=False, **REF)
    sa = WarmupCosineLR(oa, max_iters=60, warmup_factor=0.1, warmup_iters=10)
    sb = WarmupCosineLR(ob, max_iters=60, warmup_factor=0.1, warmup_iters=10)
    return pa, pb, oa, ob, sa, sb


def _run(pa, pb, oa, ob, sa, sb, steps, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for _ in range(steps):
        for a, b in zip(pa, pb):
            gr = torch.randn(a.shape, generator=g, device="cuda")
            a.grad, b.grad = gr.clone(), gr.clone()
        oa.step()
        ob.step()
        sa.step()
        sb.step()
    torch.cuda.synchronize()
    assert [gr["lr"] for gr in oa.param_groups] == [gr["lr"] for gr in ob.param_groups]


def _close(pa, pb, oa, ob, tol=1e-6):
    for a, b in zip(pa, pb):
        sa, sb = oa.state[a], ob.state[b]
        assert float(sa["step"]) == float(sb["step"])
        for x, y in ((a, b), (sa["exp_avg"], sb["exp_avg"]), (sa["exp_avg_sq"], sb["exp_avg_sq"])):
            err = (x - y).abs().max().item()
            assert err <= tol * max(y.abs().max().item(), 1e-30), (tuple(a.shape), err)


@gpu
@pytest.mark.parametrize("kind", ["AdamW", "Adam"])
def test_one_step_and_fifty_steps_match_torch(kind):
    from picopose_amd import optim

    pa, pb, oa, ob, sa, sb = _pair(getattr(optim, kind), getattr(torch.optim, kind))
    _run(pa, pb, oa, ob, sa, sb, 1, 1)
    for a, b, a0 in zip(pa, pb, _tensors(0)):
        sa_, sb_ = oa.state[a], ob.state[b]
        assert not torch.equal(a.detach(), a0.cuda())                                  # the step moved every tensor
        for x, y, what in ((a, b, "p"), (sa_["exp_avg"], sb_["exp_avg"], "m"), (sa_["exp_avg_sq"], sb_["exp_avg_sq"], "v")):
            assert _within_ulps(x.detach(), y.detach()), (kind, what, tuple(a.shape))
        assert sa_["step"].device.type == "cpu" and sa_["step"].dtype == torch.float32
    _run(pa, pb, oa, ob, sa, sb, 49, 2)
    _close(pa, pb, oa, ob)


@gpu
def test_parameters_without_gradient_are_skipped():
    from picopose_amd.optim import AdamW

    a, b = torch.nn.Parameter(torch.ones(16, device="cuda")), torch.nn.Parameter(torch.ones(16, device="cuda"))
    opt = AdamW([a, b], lr=1e-2)
    a.grad = torch.ones_like(a)
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(b.detach(), torch.ones(16, device="cuda")) and b not in opt.state
    assert float(opt.state[a]["step"]) == 1.0 and not torch.equal(a.detach(), torch.ones(16, device="cuda"))


@gpu
@pytest.mark.parametrize("kind", ["AdamW", "Adam"])
def test_state_dict_round_trip_with_torch(kind):
    from picopose_amd import optim

    for first_torch in (True, False):
        init = _tensors(3)
        mk = lambda: [torch.nn.Parameter(t.cuda()) for t in init]  # noqa: E731
        ours, theirs = getattr(optim, kind), getattr(torch.optim, kind)
        A, B = (theirs, ours) if first_torch else (ours, theirs)
        kw = lambda cls: dict(foreach=False) if cls is theirs else {}  # noqa: E731
        p0 = mk()
        o0 = A(_groups(p0), lr=1e-3, **REF, **kw(A))
        p_ref = mk()
        o_ref = A(_groups(p_ref), lr=1e-3, **REF, **kw(A))
        s0 = optim.WarmupCosineLR(o0, max_iters=60, warmup_factor=0.1, warmup_iters=3)
        s_ref = optim.WarmupCosineLR(o_ref, max_iters=60, warmup_factor=0.1, warmup_iters=3)
        _run(p0, p_ref, o0, o_ref, s0, s_ref, 5, 4)
        sd, ssd = o0.state_dict(), s0.state_dict()
        assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
        # hand over: a fresh model copy with the other optimizer continues
        p1 = [torch.nn.Parameter(p.detach().clone()) for p in p0]
        o1 = B(_groups(p1), lr=1e-3, **REF, **kw(B))
        s1 = optim.WarmupCosineLR(o1, max_iters=60, warmup_factor=0.1, warmup_iters=3)
        o1.load_state_dict(sd)          # (a resume: optimizer and scheduler built first, then both states loaded)
        s1.load_state_dict(ssd)
        assert [g["lr"] for g in o1.param_groups] == [g["lr"] for g in o_ref.param_groups]
        _run(p1, p_ref, o1, o_ref, s1, s_ref, 5, 5)
        _close(p1, p_ref, o1, o_ref)


def _seed(i):
    """The training forward draws the stage-2 pose noise (utils/augment.aug_gtM_noise) from numpy and torch: the same draws for both runs."""
    import numpy as np

    np.random.seed(i)
    torch.manual_seed(i)


def _split_ref(w, t):
    """(hl, scale2) of a fresh pp_split_weights_ws of w."""
    from picopose_amd import _lib
    from picopose_amd.ops import _p

    hl = torch.empty(w.shape[0], t * w.shape[1], dtype=torch.float16, device=w.device)
    buf = torch.empty(2 + 1024, dtype=torch.float32, device=w.device)
    _lib.check(_lib.lib().pp_split_weights_ws(_p(w), w.numel(), t, _p(hl), _p(buf), _p(buf[2:]), _lib.stream_ptr()), "split")
    return hl, buf[:2]


class _CountSplits:
    def __init__(self, monkeypatch):
        from picopose_amd import _lib

        L = _lib.lib()
        orig = L.pp_split_weights_ws
        self.ptrs = []

        def wrapped(w, *a):
            self.ptrs.append(w.value if hasattr(w, "value") else int(w))
            return orig(w, *a)

        monkeypatch.setattr(L, "pp_split_weights_ws", wrapped)


@gpu
def test_step_writes_the_split_of_every_trained_linear_at_vits(golden_dir, monkeypatch):
    from picopose_amd import ops
    from picopose_amd.optim import AdamW
    from picopose_amd.picopose import Net
    from picopose_amd.utils.loss_utils import Loss
    from netcfg import small_cfg
    from test_train_gpu import _cuda, _load_grad_fixture

    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    ops.drop_split_cache()
    z, ep, weights = _load_grad_fixture(golden_dir)
    net = Net(small_cfg())
    net.load_state_dict(weights(net.state_dict()))
    net = net.cuda().train()
    ep = _cuda(ep)
    Loss()(net(dict(ep)))["loss"].backward()
    trained = [p for p in net.parameters() if p.grad is not None]
    opt = AdamW(trained, lr=1e-3, betas=(0.5, 0.999), eps=1e-6, weight_decay=5e-4)
    targets, _ = ops.device_split_targets(trained)
    assert len(targets) >= 40, len(targets)            # every ViT block's qkv / proj / fc1 / fc2 at least
    opt.step()
    torch.cuda.synchronize()
    for i, hl, s2 in targets:
        w = trained[i]
        assert ops._split_cache[(w.data_ptr(), tuple(w.shape), 2, "dev")][3] == w._version
        rhl, rs2 = _split_ref(w.detach(), 2)
        assert torch.equal(s2, rs2), (tuple(w.shape), s2, rs2)
        assert torch.equal(hl.view(torch.int16), rhl.view(torch.int16)), tuple(w.shape)
    opt.zero_grad()
    count = _CountSplits(monkeypatch)
    Loss()(net(dict(ep)))["loss"].backward()
    split_now = set(count.ptrs)
    assert not split_now & {trained[i].data_ptr() for i, _, _ in targets}


@gpu
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_step_split_in_the_other_engine_formats(precision, monkeypatch):
    """f16 (one term per element, "h" format): the same bit-identity on parameters whose operands the engine cached with split_weight_dev;
    f32: the engine has no operands, and the step splits nothing."""
    from picopose_amd import ops
    from picopose_amd.optim import AdamW

    monkeypatch.setattr(ops, "PRECISION", precision)
    ops.drop_split_cache()
    g = torch.Generator().manual_seed(7)
    ps = [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.05).cuda()) for s in ((384, 1152), (1536, 384), (384,), (64, 24))]
    if precision == "f16":
        for p in ps:
            if p.dim() == 2:
                ops.split_weight_dev(p)
    targets, _ = ops.device_split_targets(ps)
    assert len(targets) == (3 if precision == "f16" else 0)
    opt = AdamW(ps, lr=1e-3, betas=(0.5, 0.999), eps=1e-6, weight_decay=5e-4)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).cuda()
    count = _CountSplits(monkeypatch)
    opt.step()
    torch.cuda.synchronize()
    assert count.ptrs == []
    for i, hl, s2 in targets:
        w = ps[i]
        rhl, rs2 = _split_ref(w.detach(), 1)
        assert torch.equal(s2, rs2) and torch.equal(hl.view(torch.int16), rhl.view(torch.int16)), tuple(w.shape)
        count.ptrs.clear()                            # (_split_ref's own launch)
        hit_hl, _ = ops.split_weight_dev(w)           # a cache hit: no launch
        assert hit_hl is hl and count.ptrs == []


@gpu
def test_adamw_with_warmup_cosine_on_the_slice(golden_dir):
    """run_train.py:109-130 on the ViT-S slice with the reference's optimizer and schedule: five AdamW steps at lr 1e-5 lower the total
    loss, follow torch.optim.AdamW to 1e-5 of each tensor's max, and a forward after the last step equals the forward of a fresh Net
    built from the updated state_dict, bit for bit (the operands the step split are the operands a fresh split makes)."""
    from picopose_amd.optim import AdamW, WarmupCosineLR
    from picopose_amd.picopose import Net
    from picopose_amd.utils.loss_utils import Loss
    from netcfg import small_cfg
    from test_train_gpu import _cuda, _load_grad_fixture

    z, ep, weights = _load_grad_fixture(golden_dir)
    ep = _cuda(ep)

    def loop(cls, **kw):
        net = Net(small_cfg())
        net.load_state_dict(weights(net.state_dict()))
        net = net.cuda().train()
        net.train_backward = "vit+stage2"
        opt = sched = None
        totals = []
        for _ in range(5):
            _seed(0)            # (one batch: the same pose-noise draws every step)
            total = Loss()(net(dict(ep)))["loss"]
            totals.append(float(total.detach()))
            total.backward()
            if opt is None:
                opt = cls([p for p in net.parameters() if p.grad is not None], lr=1e-5, betas=(0.5, 0.999), eps=1e-6,
                          weight_decay=5e-4, **kw)
                sched = WarmupCosineLR(opt, max_iters=400000, warmup_factor=0.001, warmup_iters=0)
            opt.step()
            sched.step()
            opt.zero_grad(set_to_none=True)
        return net, totals

    net, totals = loop(AdamW)
    ref, _ = loop(torch.optim.AdamW, foreach=True)
    _seed(0)
    final = float(Loss()(net(dict(ep)))["loss"].detach())
    print("slice total loss over five AdamW steps:", [round(v, 5) for v in totals], "->", round(final, 5))
    assert final < totals[0], (totals, final)
    rp = dict(ref.named_parameters())
    for name, p in net.named_parameters():
        err = (p.detach() - rp[name].detach()).abs().max().item()
        assert err <= 1e-5 * max(rp[name].detach().abs().max().item(), 1e-30), (name, err)
    fresh = Net(small_cfg())
    fresh.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    fresh = fresh.cuda().train()
    fresh.train_backward = "vit+stage2"
    _seed(6)
    a = net(dict(ep))
    _seed(6)
    b = fresh(dict(ep))
    keys = [k for k in a if k.startswith("loss")]
    assert keys
    for k in keys:
        assert torch.equal(a[k].detach(), b[k].detach()), (k, float(a[k]), float(b[k]))
