"""The sampling, normalisation and layout kernels through picopose_amd.ops / .autograd (and _lib where ops cannot express the case)
against the float64 references and derived element-wise bounds of tests/kernel_bounds.py, over the sweep of shapes and edges where
their paths switch.  Every case prints one [bound] line; the layout kernels are bit-equal to torch indexing.  feat of the warp is
always a fresh contiguous tensor: the kernel reads it in 16-byte vectors and its entry point does not check that alignment."""
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_bounds as kb  # noqa: E402

gpu = pytest.mark.gpu
ACT_ID = {"relu": 1, "gelu": 2, "leaky01": 3, "tanh": 4}


def _cuda(inp):
    return {k: v.cuda() for k, v in inp.items()}


def _unsplit(sp):
    """fp32 value of an operand buffer: (hi + lo) / 4 (hl format: per 8 channels 8 hi then 8 lo terms) or hi / 4 (h format)"""
    hl = sp.hl.float().cpu()
    rows = hl.shape[0]
    if sp.terms == 2:
        v = hl.view(rows, -1, 2, 8)
        return ((v[:, :, 0] + v[:, :, 1]) / 4.0).reshape(rows, -1)
    return hl / 4.0


def _bn_holder(t):
    hb = types.SimpleNamespace()
    hb.weight, hb.bias = t["gamma"], t["beta"]
    hb.running_mean, hb.running_var = t["running_mean"].clone(), t["running_var"].clone()
    hb.num_batches_tracked = torch.zeros((), dtype=torch.long, device="cuda")
    return hb


def _grads(fn, tensors, dy):
    xs = [t.clone().requires_grad_(True) for t in tensors]
    fn(*xs).backward(dy)
    return tuple(x.grad for x in xs)


def run_hip(op, c, inp):
    """the operation's outputs from the HIP kernels, in the structure kernel_bounds.model returns"""
    from picopose_amd import _lib, ops
    from picopose_amd import autograd as ag

    t = _cuda(inp)
    L = _lib.lib()
    if op == "resize":
        return ops.resize_bilinear(t["x"], c["Ho"], c["Wo"], mul=c["mul"])
    if op == "warp":
        B, H, W, C = c["B"], c["H"], c["W"], c["C"]
        wide = torch.full((B, H, W, C + 8), 7.5, device="cuda")            # out as a channel slice, canaries left and right
        out = ops.warp(t["feat"], t["flow"][..., :2] if c["ld_flow"] > 2 else t["flow"], out=wide[..., 4:4 + C])
        assert bool((wide[..., :4] == 7.5).all()) and bool((wide[..., 4 + C:] == 7.5).all()), "warp wrote outside its channel slice"
        return out
    if op == "avgpool2":
        return ops.avgpool2(t["x"])
    if op == "layernorm":
        return ops.layernorm(t["x"], t["gamma"], t["beta"], kb.EPS[op])
    if op == "groupnorm":
        B, HW, C = c["B"], c["HW"], c["C"]
        return ops.groupnorm(t["x"].view(B, HW, 1, C), t["gamma"], t["beta"], c["G"], relu=c["relu"]).view(B, HW, C)
    if op == "batchnorm":
        hb = _bn_holder(t)
        y = ops.batchnorm_train(t["x"].view(1, 1, c["rows"], c["C"]), hb, relu=c["relu"], residual=t["res1"].view(1, 1, c["rows"], c["C"]) if "res1" in t else None,
                                residual2=t["res2"].view(1, 1, c["rows"], c["C"]) if "res2" in t else None)
        assert int(hb.num_batches_tracked) == 1
        return y.view(c["rows"], c["C"]), hb.running_mean, hb.running_var
    if op == "softmax":
        return ops.softmax_rows_(t["x"].clone())
    if op == "normalize":
        return ops.normalize_rows(t["x"])
    if op == "assemble":
        return ops.assemble_tokens(t["patches"], t["cls"], t["pos"])
    if op == "act":
        y = torch.empty_like(t["z"])
        _lib.check(L.pp_act_forward(t["z"].data_ptr(), c["n"], ACT_ID[c["act"]], y.data_ptr(), _lib.stream_ptr()), "pp_act_forward")
        return y
    if op == "elementwise":
        return ag._ew(c["op"], t["a"], t["v"] if c["op"] == 1 else t["b"], c["cols"])
    if op == "colsum":
        return ag.colsum(t["x"])
    if op == "layernorm_bwd":
        return _grads(lambda x, g, b: ag.layernorm(x, g, b, kb.EPS[op]), (t["x"], t["gamma"], t["beta"]), t["dy"])
    if op == "groupnorm_bwd":
        B, HW, C = c["B"], c["HW"], c["C"]
        dx, dg, db = _grads(lambda x, g, b: ag._GroupNormRelu.apply(x, g, b, c["G"], c["relu"]), (t["x"].view(B, HW, 1, C), t["gamma"], t["beta"]),
                            t["dy"].view(B, HW, 1, C))
        return dx.view(B, HW, C), dg, db
    if op == "batchnorm_bwd":
        hb = _bn_holder(t)
        shape = (1, 1, c["rows"], c["C"])
        dx, dg, db = _grads(lambda x, g, b: ag._BatchNormTrain.apply(x, g, b, hb, c["relu"]), (t["x"].view(shape), t["gamma"], t["beta"]), t["dy"].view(shape))
        return dx.view(c["rows"], c["C"]), dg, db
    if op == "softmax_bwd":
        p = torch.softmax(t["x"].double(), 1).float()
        ds = torch.empty_like(p)
        _lib.check(L.pp_softmax_backward_rows(p.data_ptr(), t["dp"].data_ptr(), c["rows"], c["n"], ds.data_ptr(), _lib.stream_ptr()), "pp_softmax_backward_rows")
        return ds
    if op == "normalize_bwd":
        return _grads(lambda x: ag._NormalizeRows.apply(x, 1e-12), (t["x"],), t["dq"])[0]
    if op == "resize_bwd":
        return _grads(lambda x: ag.resize(x, c["Ho"], c["Wo"], c["mul"]), (t["x"],), t["dy"])[0]
    if op == "avgpool2_bwd":
        dx = torch.empty_like(t["x"])
        _lib.check(L.pp_avgpool2_backward_nhwc(t["dy"].data_ptr(), c["B"], c["H"], c["W"], c["C"], 0, dx.data_ptr(), _lib.stream_ptr()), "pp_avgpool2_backward_nhwc")
        return dx
    if op == "warp_bwd":
        return _grads(lambda f, fl: ag._Warp.apply(f, fl), (t["feat"], t["flow"]), t["dy"])
    if op == "act_bwd":
        return _grads(lambda z: ag._Act.apply(z, c["act"]), (t["z"],), t["dy"])[0]
    raise ValueError(op)


@gpu
@pytest.mark.parametrize("op", kb.OPS)
def test_kernel_against_float64_bound(op):
    """Every case of the operation's sweep: |kernel - float64 reference| <= MARGIN x model, element by element."""
    torch.manual_seed(0)
    for c in kb.CASES[op]:
        inp = kb.inputs(op, c)
        ref, bound = kb.reference(op, c, inp)
        got = run_hip(op, c, inp)
        name = kb.case_name(op, c)
        if isinstance(ref, tuple):
            for i, (gt, r, b) in enumerate(zip(got, ref, bound)):
                kb.check(f"{name}[{i}]", gt, r, b, op)
        else:
            if op == "softmax":      # beside -inf the probability is exactly 0
                assert bool((got.cpu()[inp["x"] == float("-inf")] == 0).all())
            kb.check(name, got, ref, bound, op)
    w = kb.eb.WORST.get(op)
    print(f"[worst] {op}: {w[0]:.3g} at {w[1]}" if w else f"[worst] {op}: -")


@gpu
def test_resize_paths_agree_and_operand_outputs():
    """The scalar path taken for a misaligned input view (C % 4 == 0) agrees bit for bit with the vector path (one blend with its
    contraction spelled out, csrc/pp_sample.hip resize_blend: left to the compiler the 4-channel path fused one more multiply-add
    than the other two) and both are inside the bound; the identity
    resampling is mul * x exactly; the operand outputs (both term counts) hold the fp32 result's split within the split model and
    the dual output's fp32 map is bit-equal to the plain one."""
    from picopose_amd import ops

    g = torch.Generator().manual_seed(11)
    for (B, H, W, C, Ho, Wo, mul) in [(3, 16, 16, 12, 32, 32, 2.0), (1, 5, 7, 4, 9, 11, -0.5), (2, 64, 64, 8, 37, 37, 1.0)]:
        x = torch.randn(B, H, W, C, generator=g)
        flat = torch.empty(x.numel() + 1, device="cuda")
        flat[1:] = x.cuda().reshape(-1)
        xv = flat[1:].view(B, H, W, C)
        assert xv.data_ptr() % 16 != 0 and xv.is_contiguous()
        c = dict(B=B, H=H, W=W, C=C, Ho=Ho, Wo=Wo, mul=mul)
        ref, bound = kb.reference("resize", c, dict(x=x))
        scalar, vector = ops.resize_bilinear(xv, Ho, Wo, mul=mul), ops.resize_bilinear(x.cuda(), Ho, Wo, mul=mul)
        print(f"[paths] resize {c}: scalar vs vector path max |diff| = {float((scalar - vector).abs().max()):.3g}", flush=True)
        assert torch.equal(scalar, vector)
        kb.check(f"resize scalar path (misaligned view) {c}", scalar, ref, bound, "resize")
        kb.check(f"resize vector path {c}", vector, ref, bound, "resize")
    x = torch.randn(2, 8, 8, 8, generator=g).cuda()
    for mul in (1.0, 2.0, -0.5):
        assert torch.equal(ops.resize_bilinear(x, 8, 8, mul=mul), x * mul)
    for (H, Ho, C) in [(16, 32, 8), (32, 64, 256), (8, 1, 8)]:
        c = dict(H=H, W=H, Ho=Ho, Wo=Ho, C=C, mul=1.0, B=2)
        inp = kb.inputs("resize", c, seed=5)
        plain = ops.resize_bilinear(inp["x"].cuda(), Ho, Ho)
        for mode, terms in (("f16x3", 2), ("f16", 1)):
            with ops.precision_scope(mode):
                sp = ops.resize_bilinear(inp["x"].cuda(), Ho, Ho, out_split=True)
                dual = ops.resize_bilinear(inp["x"].cuda(), Ho, Ho, also_split=True)
            assert isinstance(sp, ops.Split) and sp.terms == terms
            assert torch.equal(dual, plain) and torch.equal(dual._hl.hl, sp.hl)
            ref, bound = kb.reference("resize", c, inp, terms=terms)
            kb.check(f"resize operand terms={terms} {H}->{Ho} C={C}", _unsplit(sp).view(ref.shape), ref, bound, "resize")


@gpu
def test_warp_edges():
    """Exact-integer flows (sizes whose size - 1 is a power of two, so that the coordinate round trip is exact: weights 0 / 1) are
    bit-equal to indexing with zeros outside; flows of +-1e30, inf and nan give finite zeros (the kernel clamps the coordinate
    before the integer conversion); an inf in a pixel only out-of-image taps touch never enters; the operand-column output equals
    the split of the fp32 result within the split model; the deterministic adjoint repeats bit for bit."""
    from picopose_amd import autograd as ag
    from picopose_amd import ops

    for c in [k for k in kb.CASES["warp"] if k["kind"] == "integer"]:
        inp = kb.inputs("warp", c)
        B, H, W, C = c["B"], c["H"], c["W"], c["C"]
        got = ops.warp(inp["feat"].cuda(), inp["flow"].cuda()).cpu()
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        tx, ty = xs + inp["flow"][..., 0].long(), ys + inp["flow"][..., 1].long()
        ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        feat = inp["feat"][torch.arange(B) % c["feat_batch"]]
        want = feat[torch.arange(B).view(B, 1, 1), ty.clamp(0, H - 1), tx.clamp(0, W - 1)] * ok.unsqueeze(-1)
        assert torch.equal(got, want)
    g = torch.Generator().manual_seed(3)
    B, H, W, C = 2, 8, 8, 8
    feat = torch.randn(B, H, W, C, generator=g)
    flow = torch.randn(B, H, W, 2, generator=g)
    flow[0, 0, 0, 0], flow[0, 0, 1, 1], flow[0, 1, 0, 0], flow[0, 1, 1, 1] = 1e30, -1e30, float("inf"), float("nan")
    flow[1, 2, 2] = torch.tensor([float("-inf"), float("nan")])
    got = ops.warp(feat.cuda(), flow.cuda()).cpu()
    assert bool(torch.isfinite(got).all())
    for idx in [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 2, 2)]:
        assert bool((got[idx] == 0).all()), idx
    # an inf in pixel (3, 3) of a 4 x 4 map and every target at (4.5, 4.5): all four taps lie outside and are clamped onto that pixel
    feat2 = torch.randn(1, 4, 4, 8, generator=g)
    feat2[0, 3, 3] = float("inf")
    flow2 = torch.zeros(1, 4, 4, 2)
    ys, xs = torch.meshgrid(torch.arange(4.0), torch.arange(4.0), indexing="ij")
    flow2[0, ..., 0], flow2[0, ..., 1] = 4.5 - xs, 4.5 - ys          # every target (4.5, 4.5): all four taps outside, clamped onto pixel (3, 3)
    assert bool((ops.warp(feat2.cuda(), flow2.cuda()) == 0).all())
    for c in [k for k in kb.CASES["warp"] if k["C"] % 8 == 0 and k["kind"] == "border" and k["H"] * k["W"] <= 16 * 24][:6]:
        inp = kb.inputs("warp", c)
        rows = c["B"] * c["H"] * c["W"]
        for mode, terms in (("f16x3", 2), ("f16", 1)):
            with ops.precision_scope(mode):
                tgt = ops.Split(torch.full((rows, terms * (c["C"] + 16)), 3.0, dtype=torch.float16, device="cuda"))
                ops.warp(inp["feat"].cuda(), inp["flow"][..., :2].cuda() if c["ld_flow"] > 2 else inp["flow"].cuda(), hl_into=(tgt, 8))
            assert bool((tgt.cols(0, 8) == 3.0).all()) and bool((tgt.cols(8 + c["C"], 8) == 3.0).all()), "operand columns outside the slice written"
            ref, bound = kb.reference("warp", c, inp, terms=terms)
            kb.check(f"warp operand terms={terms} {kb.case_name('warp', c)}", _unsplit(ops.Split(tgt.cols(8, c["C"]).contiguous(), terms)).view(ref.shape),
                     ref, bound, "warp")
    c = kb.CASES["warp_bwd"][-1]
    inp = kb.inputs("warp_bwd", c)
    old = ag.DETERMINISTIC
    try:
        ag.DETERMINISTIC = True
        runs = [_grads(lambda f, fl: ag._Warp.apply(f, fl), (inp["feat"].cuda(), inp["flow"].cuda()), inp["dy"].cuda()) for _ in range(2)]
    finally:
        ag.DETERMINISTIC = old
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ref, bound = kb.reference("warp_bwd", c, inp)
    kb.check("warp_bwd fixed-point dfeat", runs[0][0], ref[0], bound[0] + 2.0 ** -40 * 16, "warp_bwd")   # (+ the 2^-40 grid of the accumulators)
    kb.check("warp_bwd fixed-point dflow", runs[0][1], ref[1], bound[1], "warp_bwd")


@gpu
def test_layernorm_operand_output_and_misaligned_gamma():
    """The operand output (both term counts) within the split model of the bounded fp32 result; a gamma view that is not 16-byte
    aligned takes the any-width instance and must agree with the register-resident one to the bound."""
    from picopose_amd import ops

    for c in [dict(rows=5, C=384, offset=10), dict(rows=257, C=1024, offset=0), dict(rows=4, C=2048, offset=0), dict(rows=3, C=40, offset=100)]:
        inp = kb.inputs("layernorm", c, seed=9)
        t = _cuda(inp)
        for mode, terms in (("f16x3", 2), ("f16", 1)):
            with ops.precision_scope(mode):
                sp = ops.layernorm(t["x"], t["gamma"], t["beta"], 1e-6, out_split=True)
            assert isinstance(sp, ops.Split) and sp.terms == terms
            ref, bound = kb.reference("layernorm", c, inp, terms=terms)
            kb.check(f"layernorm operand terms={terms} {c}", _unsplit(sp), ref, bound, "layernorm")
        flat = torch.empty(c["C"] + 1, device="cuda")
        flat[1:] = t["gamma"]
        assert flat[1:].data_ptr() % 16 != 0
        ref, bound = kb.reference("layernorm", c, inp)
        kb.check(f"layernorm misaligned gamma {c}", ops.layernorm(t["x"], flat[1:], t["beta"], 1e-6), ref, bound, "layernorm")


@gpu
def test_softmax_rows_with_a_gap_between_rows():
    """ld > n through the C ABI: the rows are bounded like the dense ones and the gap's canaries stay intact."""
    from picopose_amd import _lib

    for c in [dict(rows=5, n=63, scale=1.0), dict(rows=1028, n=65, scale=30.0), dict(rows=3, n=1, scale=1.0), dict(rows=7, n=257, scale=1.0)]:
        inp = kb.inputs("softmax", c, seed=2)
        ld = c["n"] + 5
        buf = torch.full((c["rows"], ld), -7.0, device="cuda")
        buf[:, :c["n"]] = inp["x"].cuda()
        _lib.check(_lib.lib().pp_softmax_rows(buf.data_ptr(), c["rows"], c["n"], ld, _lib.stream_ptr()), "pp_softmax_rows")
        assert bool((buf[:, c["n"]:] == -7.0).all())
        ref, bound = kb.reference("softmax", c, inp)
        kb.check(f"softmax ld={ld} {c}", buf[:, :c["n"]], ref, bound, "softmax")


@gpu
def test_layout_kernels_are_bit_equal_to_torch_indexing():
    """to_nhwc (with and without c_pad: the padding channels exactly zero), to_nchw, tokens_to_nchw (skip 0, 1, 5), gather_rows with
    repeated and out-of-order indices; pp_transpose_batched into a wider destination leaves the canary columns and rows alone."""
    from picopose_amd import _lib, ops

    g = torch.Generator().manual_seed(17)
    for C in [1, 3, 31, 32, 33, 256]:
        for HW in [1, 31, 33, 1024]:
            H, W = (1, HW) if HW < 1024 else (32, 32)
            x = torch.randn(2, C, H, W, generator=g)
            assert torch.equal(ops.to_nhwc(x.cuda()).cpu(), x.permute(0, 2, 3, 1).contiguous())
            Cp = -(-(C + 1) // 8) * 8
            y = ops.to_nhwc(x.cuda(), c_pad=Cp).cpu()
            assert torch.equal(y[..., :C], x.permute(0, 2, 3, 1)) and bool((y[..., C:] == 0).all())
            assert torch.equal(ops.to_nchw(x.permute(0, 2, 3, 1).contiguous().cuda()).cpu(), x)
            # canaries: the destination is the middle of a wider, taller buffer
            R, Cc = C, H * W
            big = torch.full((2, Cc + 2, R + 6), 9.0, device="cuda")
            _lib.check(_lib.lib().pp_transpose_batched(x.cuda().data_ptr(), 0, 2, R, Cc, big[:, 1].data_ptr(), (Cc + 2) * (R + 6), R + 6, 3,
                                                       _lib.stream_ptr()), "pp_transpose_batched")
            assert torch.equal(big[:, 1:Cc + 1, 3:3 + R].cpu(), x.view(2, R, Cc).transpose(1, 2))
            big[:, 1:Cc + 1, 3:3 + R] = 9.0
            assert bool((big == 9.0).all()), "pp_transpose_batched wrote outside its destination"
    for skip in (0, 1, 5):
        for (H, W, C) in [(1, 1, 8), (3, 5, 33), (16, 16, 384)]:
            tok = torch.randn(2, skip + H * W, C, generator=g)
            assert torch.equal(ops.tokens_to_nchw(tok.cuda(), skip, H, W).cpu(), tok[:, skip:].transpose(1, 2).reshape(2, C, H, W))
    src = torch.randn(11, 3, 4, generator=g)
    idx = torch.tensor([10, 0, 0, 7, 3, 10, 1])
    assert torch.equal(ops.gather_rows(src.cuda(), idx.cuda()).cpu(), src[idx])


@gpu
def test_batchnorm_biased_in_the_output_unbiased_in_the_running_variance():
    """Asserted separately from the bound: the normalisation uses the biased variance, running_var the unbiased one."""
    c = dict(rows=3, C=8, relu=False, res=0, offset=0)
    inp = kb.inputs("batchnorm", c)
    y, rm, rv = run_hip("batchnorm", c, inp)
    x = inp["x"].double()
    var_b, var_u = x.var(0, unbiased=False), x.var(0, unbiased=True)
    want = (x - x.mean(0)) / torch.sqrt(var_b + 1e-5) * inp["gamma"].double() + inp["beta"].double()
    assert float((y.cpu().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
    assert torch.allclose(rv.cpu().double(), 0.9 * inp["running_var"].double() + 0.1 * var_u, rtol=1e-5, atol=0)
    assert not torch.allclose(rv.cpu().double(), 0.9 * inp["running_var"].double() + 0.1 * var_b, rtol=1e-3, atol=0)
