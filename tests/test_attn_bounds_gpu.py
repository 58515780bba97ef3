"""The fused self-attention and its adjoint on the GPU against the float64 references and element-wise bounds of tests/attn_bounds.py: attn_kernel
(f32, three- and four-wave workgroups), attn_f16x3_kernel from the fp32 qkv and from the operand ops.split_activation writes, in the f16x3 and
the f16 format, register-staged (PP_ATTN_RING=0), through the LDS-DMA ring of two and three stages and, at T = 257 and 260, resident
(PP_ATTN_RESIDENT=1); fp32 and operand output; the training forward with its log-sum-exp; the recomputing adjoint (dq, dk, dv each to its own
bound, two runs bit-equal); the unfused chain (batched GEMMs and the soft-max row kernels) against the same references.  Every path has its own
[worst] key, printed after the last test of the file.  The references are computed in this process on the CPU from torch's float64 ops."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_bounds as ab  # noqa: E402

gpu = pytest.mark.gpu
HD = ab.HD


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios_summary():
    """after the last test of this file that ran: the worst |err| / bound per path (the figures of DESIGN.md)"""
    yield
    for key, (worst, where) in sorted(ab.eb.WORST.items()):
        if key.split()[0] in ("attn", "attn_lse", "attn_bwd"):
            print(f"[worst] {key}: {worst:.3g} at {where}", flush=True)


def _ids(op):
    return [ab.case_id(c) for c in ab.CASES[op]]


def _env(monkeypatch, ring):
    """ring: "0" | "2" | "3" | "res" (the resident variant: opt-in on top of a ring setting)"""
    monkeypatch.setenv("PP_ATTN_RING", "2" if ring == "res" else ring)
    if ring == "res":
        monkeypatch.setenv("PP_ATTN_RESIDENT", "1")
    else:
        monkeypatch.delenv("PP_ATTN_RESIDENT", raising=False)


@gpu
@pytest.mark.parametrize("c", ab.CASES["attn"], ids=_ids("attn"))
def test_forward_stays_inside_the_float64_bound(monkeypatch, c):
    from picopose_amd import _lib, ops

    name = ab.case_name("attn", c)
    B, T, H = c["B"], c["T"], c["heads"]
    inp = ab.inputs("attn", c)
    qkv = inp["qkv"].cuda()
    bounds = {m: ab.reference("attn", c, inp, m) for m in ab.MODES}
    monkeypatch.delenv("PP_ATTN_RING", raising=False)
    monkeypatch.delenv("PP_ATTN_RESIDENT", raising=False)
    with ops.precision_scope("f32"):
        got = ops.attention(qkv, B, T, H, HD)
    ab.check(f"{name} f32", got, *bounds["f32"], mode="attn f32")
    with ops.precision_scope("f16x3"):
        # attn_kernel's operand output (pp_attention_split): the fp32 result and its split from one launch
        o32 = torch.empty(B * T, H * HD, dtype=torch.float32, device="cuda")
        ohl = torch.empty(B * T, 2 * H * HD, dtype=torch.float16, device="cuda")
        _lib.call("pp_attention_split", qkv, B, T, H, HD, float(HD) ** -0.5, o32, ohl)
        assert torch.equal(o32, got), f"{name}: pp_attention_split differs from pp_attention"
        assert torch.equal(ohl, ops.split_activation(o32, 1, B * T, H * HD, 0, H * HD)), f"{name}: f32 kernel, operand output"
        x3 = ops.attention(qkv, B, T, H, HD)
        ab.check(f"{name} f16x3 fp32-input", x3, *bounds["f16x3"], mode="attn f16x3 fp32-input")
        sp3 = ops.attention(qkv, B, T, H, HD, out_split=True)
        assert torch.equal(sp3.hl, ops.split_activation(x3, 1, B * T, H * HD, 0, H * HD)), f"{name}: fp32 input, operand output"
    rings = ("0", "2", "3") + (("res",) if T in (257, 260) else ())
    for mode in ("f16x3", "f16"):
        with ops.precision_scope(mode):
            sp = ops.Split(ops.split_activation(qkv, 1, B * T, 3 * H * HD, 0, 3 * H * HD))
            first = None
            for ring in rings:
                _env(monkeypatch, ring)
                o = ops.attention(sp, B, T, H, HD)
                ab.check(f"{name} {mode} operand ring={ring}", o, *bounds[mode], mode=f"attn {mode} operand ring={ring}")
                osp = ops.attention(sp, B, T, H, HD, out_split=True)
                assert torch.equal(osp.hl, ops.split_activation(o, 1, B * T, H * HD, 0, H * HD)), f"{name} {mode} ring={ring}: operand output"
                if first is None:
                    first = (o, osp.hl)
                else:
                    assert torch.equal(o, first[0]) and torch.equal(osp.hl, first[1]), f"{name} {mode}: ring={ring} differs from the register-staged kernel"
            if mode == "f16x3":
                assert torch.equal(first[0], x3), f"{name}: operand input differs from the fp32-input f16x3 result"


@gpu
@pytest.mark.parametrize("c", ab.CASES["attn"], ids=_ids("attn"))
def test_training_forward_and_its_log_sum_exp(c):
    from picopose_amd import _lib, ops

    name = ab.case_name("attn", c)
    B, T, H = c["B"], c["T"], c["heads"]
    inp = ab.inputs("attn", c)
    qkv = inp["qkv"].cuda()
    out = torch.empty(B * T, H * HD, dtype=torch.float32, device="cuda")
    lse = torch.empty(B * H, T, dtype=torch.float32, device="cuda")
    _lib.call("pp_attention_train", qkv, B, T, H, HD, float(HD) ** -0.5, out, lse)
    ab.check(f"{name} train out", out, *ab.reference("attn", c, inp, "f16x3"), mode="attn f16x3 train")
    ab.check(f"{name} train lse", lse, *ab.reference("attn_lse", c, inp), mode="attn_lse")
    with ops.precision_scope("f16x3"):
        assert torch.equal(out, ops.attention(qkv, B, T, H, HD)), f"{name}: the training forward differs from the inference forward"


class _Ctx(types.SimpleNamespace):
    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


def _run(ag, qkv, dout, c):
    """_Attention forward + backward on this thread (the arithmetic mode is thread-local): (out, dq, dk, dv)"""
    B, T, H = c["B"], c["T"], c["heads"]
    ctx = _Ctx()
    out = ag._Attention.forward(ctx, qkv, B, T, H, HD)
    dqkv = ag._Attention.backward(ctx, dout)[0]
    torch.cuda.synchronize()
    C = H * HD
    return out, dqkv[:, :C], dqkv[:, C:2 * C], dqkv[:, 2 * C:]


@gpu
@pytest.mark.parametrize("c", ab.CASES["attn_bwd"], ids=_ids("attn_bwd"))
def test_adjoint_stays_inside_the_float64_bound(monkeypatch, c):
    from picopose_amd import autograd as ag
    from picopose_amd import ops

    name = ab.case_name("attn_bwd", c)
    inp = ab.inputs("attn_bwd", c)
    qkv, dout = inp["qkv"].cuda(), inp["dout"].cuda()
    ref, bound = ab.reference("attn_bwd", c, inp)
    monkeypatch.setattr(ag, "FUSED_ATTENTION", True)
    with ops.precision_scope("f16x3"):
        got = _run(ag, qkv, dout, c)
        again = _run(ag, qkv, dout, c)
    ab.check(f"{name} out", got[0], *ab.reference("attn", c, inp, "f16x3"), mode="attn f16x3 train")
    for what, g, rf, b in zip(("dq", "dk", "dv"), got[1:], ref, bound):
        ab.check(f"{name} {what}", g, rf, b, mode=f"attn_bwd {what}")
    assert all(torch.equal(a, b) for a, b in zip(got, again)), f"{name}: two runs differ"
    if c["T"] == 1:
        print(f"[T=1] {name}: max |dq| = {float(got[1].abs().max()):.3g}, max |dk| = {float(got[2].abs().max()):.3g}", flush=True)
        assert not bool(got[1].any()) and not bool(got[2].any()), f"{name}: dq and dk of a single key are not exactly 0"


@gpu
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("c", ab.UNFUSED, ids=[ab.case_id(c) for c in ab.UNFUSED])
def test_unfused_chain_against_the_same_references(monkeypatch, c, mode):
    """batched GEMMs + the soft-max row kernels: the f32 engine's route, and the f16x3 engine's with FUSED_ATTENTION off"""
    from picopose_amd import autograd as ag
    from picopose_amd import ops

    name = ab.case_name("attn_bwd", c) + " unfused " + mode
    inp = ab.inputs("attn_bwd", c)
    qkv, dout = inp["qkv"].cuda(), inp["dout"].cuda()
    # (f16x3: dS is split with one power of two for the whole tensor and P at scale 4: the chain's own model terms and margins, attn_bounds.py)
    ref, bound = ab.reference("attn_bwd", c, inp, unfused=mode == "f16x3")
    monkeypatch.setattr(ag, "FUSED_ATTENTION", False)
    with ops.precision_scope(mode):
        got = _run(ag, qkv, dout, c)
    ab.check(f"{name} out", got[0], *ab.reference("attn", c, inp, mode), mode=f"attn unfused {mode}")
    for what, g, rf, b in zip(("dq", "dk", "dv"), got[1:], ref, bound):
        ab.check(f"{name} {what}", g, rf, b, mode=f"attn_bwd unfused {mode} {what}")
