"""The selected templates' last ViT level read from the feature bank (Net.template_last_from_bank, pp_bank_rows_to_tokens) instead of
running the blocks after the second-to-last taken one on them again: the kernel against torch indexing, every forward output bit for bit
against the recomputing forward, the launch records of the engine showing that the work is gone, and the cases that keep recomputing."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from netcfg import make_end_points, small_cfg  # noqa: E402

from oracle.weights import seeded_state_dict  # noqa: E402

gpu = pytest.mark.gpu
PP_EINVAL = -1
B, N, HYP, T, C = 2, 4, 2, 257, 384          # small_cfg(): ViT-S/14 on 224 x 224 crops, depth 12, levels after blocks 2, 5, 8, 11


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("R,Cb,P,index,ld,Tt,skip,img0", [
    (7, 72, 15, [3, 6, 0, 3, 6], 80, 16, 1, 2),        # neither C nor P a multiple of the 32 x 32 tile; a repeated row, the last row
    (4, 384, 256, [2, 0, 3], 384, 257, 1, 0),          # the ViT-S level: 12 x 8 tiles per image
])
def test_bank_rows_to_tokens_equals_indexing(R, Cb, P, index, ld, Tt, skip, img0):
    from picopose_amd import ops

    g = torch.Generator().manual_seed(5)
    bank = torch.randn(R, Cb, P, generator=g).cuda()
    idx = torch.tensor(index, device="cuda")
    n, sentinel = len(index), -7.5
    buf = torch.full(((img0 + n + 1) * Tt, ld), sentinel, device="cuda")
    dst = buf[img0 * Tt:(img0 + n) * Tt]
    assert ops.bank_rows_to_tokens(bank, idx, Tt, skip=skip, out=dst) is dst
    want = torch.full_like(buf, sentinel).view(-1, Tt, ld)
    want[img0:img0 + n, :skip, :Cb] = 0
    want[img0:img0 + n, skip:skip + P, :Cb] = bank[idx].transpose(1, 2)
    assert torch.equal(buf.view(-1, Tt, ld), want)
    fresh = ops.bank_rows_to_tokens(bank, idx, Tt, skip=skip)                 # a buffer of its own: (n * T, C)
    assert fresh.shape == (n * Tt, Cb) and torch.equal(fresh.view(n, Tt, Cb)[:, :skip + P], want[img0:img0 + n, :skip + P, :Cb])
    # an index outside the bank leaves its image as it was (pp_gather_rows does the same)
    buf.fill_(sentinel)
    ops.bank_rows_to_tokens(bank, torch.tensor([R, 1, -1], device="cuda"), Tt, skip=skip, out=buf[:3 * Tt])
    got = buf.view(-1, Tt, ld)
    assert bool((got[0] == sentinel).all()) and bool((got[2:] == sentinel).all())
    assert torch.equal(got[1, skip:skip + P, :Cb], bank[1].t()) and bool((got[1, :skip, :Cb] == 0).all())


def test_bank_rows_to_tokens_is_declared_and_rejects_bad_arguments():
    """Null pointers and non-positive or inconsistent sizes give PP_EINVAL before any HIP call: no GPU needed."""
    from picopose_amd import _lib

    assert "pp_bank_rows_to_tokens" in _lib.declared_symbols()
    L = _lib.lib()
    a = (ctypes.c_float * 64)()
    p = ctypes.addressof(a)
    good = dict(bank=p, rows=7, C=72, P=15, index=p, n=5, tokens=p, ld=80, T=16, skip=1)
    call = lambda **kw: L.pp_bank_rows_to_tokens(*{**good, **kw}.values(), None)  # noqa: E731
    for name in ("bank", "index", "tokens"):
        assert call(**{name: None}) == PP_EINVAL, name
    for name in ("rows", "C", "P", "n", "T"):
        for bad in (0, -1):
            assert call(**{name: bad}) == PP_EINVAL, (name, bad)
    assert call(ld=71) == PP_EINVAL                      # rows shorter than C
    assert call(skip=-1) == PP_EINVAL
    assert call(skip=2) == PP_EINVAL                     # skip + P rows do not fit the T rows of an image
    assert call(n=65536) == PP_EINVAL                    # one grid plane per image


# ---- 2 - 4. the forward ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    """The network and its inputs, built once: two batches with the bank the net itself computes (run_test.py:120-134), per-object
    banks with an index, and the recomputing forward's outputs of every configuration (switch off) — the reference of every test below."""
    from picopose_amd import ops
    from picopose_amd.picopose import Net

    assert ops.PRECISION == "f16x3"
    net = Net(small_cfg())
    net.load_state_dict(seeded_state_dict(net.state_dict(), 17))
    net = net.cuda().eval()
    eps = []
    for seed in (91, 92):
        d = {k: v.cuda() for k, v in make_end_points(B, N, seed).items()}
        d["template_feature"] = torch.stack([net.feature_extractor(d["tem_rgb"][b])[-1] for b in range(B)])
        eps.append(d)
    O = 3
    tem = {k: v.cuda() for k, v in make_end_points(O, N, 93).items() if k.startswith("tem_")}
    tem["template_feature"] = torch.stack([net.feature_extractor(tem["tem_rgb"][o])[-1] for o in range(O)])
    real = {k: v for k, v in eps[0].items() if k.startswith("real_")}
    indexed = dict(real, **tem, template_index=torch.tensor([2, 0], device="cuda"))
    yield net, eps, indexed
    ops.saturation_raised()             # (plain seeded decoders leave the operand range: DESIGN section 4)


def _clone(outs):
    return [{k: v.clone() for k, v in o.items()} for o in outs]


def _same(a, b):
    assert len(a) == len(b) == HYP
    for h in range(HYP):
        assert set(a[h]) == set(b[h])
        for k in a[h]:
            assert torch.equal(a[h][k], b[h][k]), (h, k)


def _switch(net, value, fn):
    net.template_last_from_bank, net._query_stash = value, None
    try:
        return fn()
    finally:
        net.template_last_from_bank = None


def _runs(net, eps, indexed):
    """Every configuration of the forward -> {name: outputs}."""
    out = {}
    for batched in (True, False):
        net.batch_hypotheses = batched
        tag = "batched" if batched else "per-hypothesis"
        out[tag] = _clone(net(eps[0], HYP))
        out[tag + " indexed"] = _clone(net(indexed, HYP))
    net.batch_hypotheses = True
    out["look-ahead"] = _clone(net(eps[0], HYP, next_real_rgb=eps[1]["real_rgb"]))
    assert net._query_stash is not None
    out["follow-up"] = _clone(net(eps[1], HYP))                     # consumes the stash
    assert net._query_stash is None
    return out


@gpu
def test_forward_with_the_last_level_from_the_bank_keeps_every_bit(world):
    net, eps, indexed = world
    off = _switch(net, False, lambda: _runs(net, eps, indexed))
    for value in (None, True):                                     # auto (the forward runs in f16x3) and forced
        assert _switch(net, value, lambda: net._last_from_bank(eps[0]) and net._last_from_bank(indexed))
        on = _switch(net, value, lambda: _runs(net, eps, indexed))
        assert set(on) == set(off)
        for name in off:
            _same(on[name], off[name])


@gpu
def test_f32_forward_recomputes_unless_forced(world, monkeypatch):
    from picopose_amd import ops

    net, eps, _ = world
    monkeypatch.setattr(ops, "PRECISION", "f32")
    ep = dict(eps[0])
    ep["template_feature"] = torch.stack([net.feature_extractor(ep["tem_rgb"][b])[-1] for b in range(B)])     # the bank, built in f32
    off = _switch(net, False, lambda: _clone(net(ep, HYP)))
    assert not _switch(net, None, lambda: net._last_from_bank(ep))
    _same(_switch(net, None, lambda: _clone(net(ep, HYP))), off)    # auto: off under f32
    assert _switch(net, True, lambda: net._last_from_bank(ep))
    _same(_switch(net, True, lambda: _clone(net(ep, HYP))), off)    # forced, with the bank of the same arithmetic: the same bits
    net.precision = "f32"                                          # the model's own mode counts, not the global
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    try:
        with ops.precision_scope(net.precision):
            assert not net._last_from_bank(ep)
    finally:
        net.precision = None


def _qkv_rows(fn):
    """fn() under the engine's launch records -> M of every launch with N = 3 C, K = C (the qkv projections of the ViT blocks), in order."""
    from picopose_amd import _lib

    L, cap = _lib.lib(), 4096
    _lib.check(L.pp_prof_gemm_enable(cap), "pp_prof_gemm_enable")
    try:
        out = fn()
        torch.cuda.synchronize()
        shape, ms, fl, cnt = (ctypes.c_int * (6 * cap))(), (ctypes.c_float * cap)(), (ctypes.c_double * cap)(), ctypes.c_int()
        _lib.check(L.pp_prof_gemm_records(cap, shape, ms, fl, ctypes.byref(cnt)), "pp_prof_gemm_records")     # records of {M, N, K, ...}
    finally:
        _lib.check(L.pp_prof_gemm_enable(0), "pp_prof_gemm_enable")
    assert 0 < cnt.value < cap
    return out, [shape[6 * i] for i in range(cnt.value) if (shape[6 * i + 1], shape[6 * i + 2]) == (3 * C, C)]


def _look_ahead(net, eps, value):
    """One forward of batch 0 with batch 1's crops as look-ahead, its own query levels taken from the stash of the call before -> the qkv
    launches of that forward: only the template pass [look-ahead queries ; templates] runs the ViT."""
    def fn():
        net(eps[1], HYP, next_real_rgb=eps[0]["real_rgb"])
        return _qkv_rows(lambda: net(eps[0], HYP, next_real_rgb=eps[1]["real_rgb"]))
    return _switch(net, value, fn)


@gpu
def test_the_templates_last_blocks_are_not_launched(world):
    net, eps, _ = world
    Bn, full = B, (B + HYP * B) * T
    _, rows = _look_ahead(net, eps, None)
    assert rows == [full] * 9 + [Bn * T] * 3                        # blocks 9 - 11: the look-ahead queries only
    _, rows = _look_ahead(net, eps, False)
    assert rows == [full] * 12
    # without look-ahead: the query pass (12 launches of B T rows), then the template pass, which stops after block 8
    _, rows = _switch(net, None, lambda: _qkv_rows(lambda: net(eps[0], HYP)))
    assert rows == [B * T] * 12 + [HYP * B * T] * 9
    _, rows = _switch(net, False, lambda: _qkv_rows(lambda: net(eps[0], HYP)))
    assert rows == [B * T] * 12 + [HYP * B * T] * 12


@gpu
def test_fp16_bank_and_extended_bank_keep_their_paths(world):
    """A bank stored in fp16 is not the fp32 level: the forward recomputes (12 full launches) whatever the switch says.  With the extended
    bank (template_cache) no template ViT runs at all, with the switch on or off: the same launches, the same outputs."""
    net, eps, _ = world
    half = dict(eps[0], template_feature=eps[0]["template_feature"].half())
    off = _switch(net, False, lambda: _clone(net(half, HYP)))
    for value in (None, True):
        assert not _switch(net, value, lambda: net._last_from_bank(half))
        out, rows = _look_ahead(net, [half, eps[1]], value)
        assert rows == [(B + HYP * B) * T] * 12
        _same(out, off)
    banks = [net.precompute_templates(eps[0]["tem_rgb"][b]) for b in range(B)]
    ext = dict(eps[0], template_feature=torch.stack([bk["feature"] for bk in banks]),
               template_cache={"obj_index": torch.arange(B, device="cuda"), "dpt": [torch.stack([bk["dpt"][k] for bk in banks]) for k in range(3)]})
    off, rows_off = _switch(net, False, lambda: _qkv_rows(lambda: _clone(net(ext, HYP))))
    assert rows_off == [B * T] * 12                                 # the query pass alone
    for value in (None, True):
        assert not _switch(net, value, lambda: net._last_from_bank(ext))
        out, rows = _switch(net, value, lambda: _qkv_rows(lambda: _clone(net(ext, HYP))))
        assert rows == rows_off
        _same(out, off)
