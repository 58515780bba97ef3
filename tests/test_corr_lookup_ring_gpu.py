"""The ring-staged correlation lookup (per-level regions, LDS-DMA; PP_CORR_RING) against the register-staged kernel bit for bit and against
the CPU oracle; the lookup's operand output and pp_avgpool2_hl (PP_CORR_OPERAND_OUT) against the split passes they replace, bit for bit,
with the saturation report."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import nets as on  # noqa: E402

gpu = pytest.mark.gpu

# (H, W, levels, C, B): a single tile with a ring longer than the K loop (C = 32: two K steps); one level; the once-pooled region; all three
# regions; the workload's channel count; non-square
SHAPES = [(8, 8, 1, 32, 3), (16, 16, 1, 64, 3), (32, 32, 2, 64, 3), (64, 64, 3, 64, 2), (16, 16, 1, 256, 3), (16, 32, 2, 64, 3)]
FLOWS = ["smooth", "noisy", "plus_border", "minus_border", "far", "integer"]


def _flow(kind, B, H, W, g):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    smooth = torch.stack([0.15 * xx - 0.1 * yy + 1.3, 0.1 * xx + 0.2 * yy - 2.1], dim=-1)[None].repeat(B, 1, 1, 1)
    if kind == "smooth":                       # one pass per tile and level
        return smooth
    if kind == "noisy":                        # several passes at the narrowed regions
        return smooth + 3.0 * torch.randn(B, H, W, 2, generator=g)
    if kind in ("plus_border", "minus_border"):   # tile footprints straddle every image border
        s = 1.0 if kind == "plus_border" else -1.0
        return smooth * 0.0 + s * torch.tensor([W - 2.0, H - 2.0])
    if kind == "far":                          # no pass at all: zeros
        return smooth * 0.0 + 1.0e4
    return smooth * 0.0 + torch.tensor([3.0, -2.0])   # exactly-integer sample points


def _operands(ops, f1, f2):
    B, H, W, C = f1.shape
    wide = ops.Split.empty(B * H * W, 96 if C <= 64 else C + 32, f1.device)   # f1 as columns 32.. of a wider operand
    wide.hl.zero_()
    ops.split_activation(f1, B, H * W, C, H * W * C, C, into=(wide, 32))
    f2s = ops.Split(ops.split_activation(f2, f2.shape[0], H * W, C, H * W * C, C))
    return dict(f1_hl=(wide, 32), f2_hl=f2s)


def _pad_cols(n, pad):
    return [(ch >> 3) * 16 + (ch & 7) + 8 * t for ch in range(n, pad) for t in (0, 1)]


@gpu
@pytest.mark.parametrize("flow_kind", FLOWS)
@pytest.mark.parametrize("H,W,levels,C,B", SHAPES)
def test_ring_lookup_equals_the_register_staged_kernel_and_the_oracle(monkeypatch, H, W, levels, C, B, flow_kind):
    from picopose_amd import ops

    g = torch.Generator().manual_seed(H * 100 + W + levels + C)
    f1 = torch.randn(B, H, W, C, generator=g).cuda()
    f2 = torch.randn(1, H, W, C, generator=g).cuda()                       # every image reads the one query map (b % f2_batch)
    flow = _flow(flow_kind, B, H, W, g).cuda().contiguous()
    n, pad = levels * 25, -(-(levels * 25) // 8) * 8
    hl = _operands(ops, f1, f2)
    assert ops.corr_takes_operands(hl["f1_hl"], hl["f2_hl"], H, W, C)
    monkeypatch.setenv("PP_CORR_RING", "1")
    ring = ops.corr_lookup(None, f2, flow, levels, 2, c_pad=pad, **hl)
    ring_op = ops.corr_lookup(None, f2, flow, levels, 2, c_pad=pad, out_split=True, **hl)
    monkeypatch.setenv("PP_CORR_RING", "0")
    old = ops.corr_lookup(None, f2, flow, levels, 2, c_pad=pad, **hl)
    old_op = ops.corr_lookup(None, f2, flow, levels, 2, c_pad=pad, out_split=True, **hl)
    monkeypatch.setenv("PP_CORR_OPERAND_OUT", "0")                           # avgpool2 -> split_activation, fp32 map -> split_activation
    plain = ops.corr_lookup(None, f2, flow, levels, 2, c_pad=pad, **hl)
    plain_op = ops.corr_lookup(None, f2, flow, levels, 2, c_pad=pad, out_split=True, **hl)
    assert torch.equal(ring, old) and torch.equal(old, plain)
    assert torch.equal(ring[..., n:], torch.zeros_like(ring[..., n:]))
    # the operand output: the bits of the fp32 map going through the split pass, pad channels included
    want = ops.split_activation(ring, B, H * W, pad, H * W * pad, pad)
    assert ring_op.image == (B, H, W) and tuple(ring_op.hl.shape) == (B * H * W, 2 * pad)
    assert torch.equal(ring_op.hl, want) and torch.equal(old_op.hl, want) and torch.equal(plain_op.hl, want)
    if pad > n:
        cols = torch.tensor(_pad_cols(n, pad), device=want.device)
        assert int(ring_op.hl[:, cols].view(torch.int16).abs().max()) == 0
    ref = on.corr_lookup(f1.cpu().permute(0, 3, 1, 2), f2.cpu().repeat(B, 1, 1, 1).permute(0, 3, 1, 2), flow.cpu().permute(0, 3, 1, 2), levels, 2)
    ref = ref.permute(0, 2, 3, 1)
    assert float((ring[..., :n].cpu() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    if flow_kind == "far":
        assert not bool(ring.any())


@gpu
@pytest.mark.parametrize("big", [False, True])
def test_operand_output_raises_the_saturation_word_exactly_when_the_split_pass_does(monkeypatch, big):
    """|corr| beyond the fp16 range of the scaled value (4 |corr| >= 65504) with operands well inside it: the word is raised by the lookup's
    operand output exactly when the split pass of the fp32 map raises it."""
    from picopose_amd import ops

    B, H, W, C = 3, 16, 16, 64
    g = torch.Generator().manual_seed(5)
    amp = 100.0 if big else 1.0                  # <f1, f2> / sqrt(C) = 1e4 sqrt(64) = 8e4 > 16376
    f1 = (amp * (1.0 + 0.01 * torch.randn(B, H, W, C, generator=g))).cuda()
    f2 = (amp * (1.0 + 0.01 * torch.randn(1, H, W, C, generator=g))).cuda()
    flow = _flow("smooth", B, H, W, g).cuda().contiguous()
    hl = _operands(ops, f1, f2)
    ops.saturation_raised()                      # (clear whatever an earlier test left)
    for ring in ("1", "0"):
        monkeypatch.setenv("PP_CORR_RING", ring)
        out = ops.corr_lookup(None, f2, flow, 1, 2, c_pad=32, **hl)
        assert not ops.saturation_raised()       # an fp32 map reports nothing
        assert (float(out.abs().max()) * 4 >= 65504) == big
        want = ops.split_activation(out, B, H * W, 32, H * W * 32, 32)
        assert ops.saturation_raised() == big
        got = ops.corr_lookup(None, f2, flow, 1, 2, c_pad=32, out_split=True, **hl)
        assert ops.saturation_raised() == big
        assert torch.equal(got.hl, want)


@gpu
@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("H,W", [(8, 8), (16, 32)])
def test_avgpool2_hl_equals_pool_then_split(H, W, C):
    from picopose_amd import ops

    g = torch.Generator().manual_seed(H + W + C)
    x = torch.randn(2, H, W, C, generator=g).cuda()
    x[0, 0, 0, 0] = 1.0e5                         # one pooled value beyond the operand range: the same clamp, the same report
    ops.saturation_raised()                       # (clear whatever an earlier test left)
    pool = ops.avgpool2(x)
    assert not ops.saturation_raised()
    want = ops.split_activation(pool, 2, (H // 2) * (W // 2), C, (H // 2) * (W // 2) * C, C)
    assert ops.saturation_raised()
    out, sp = ops.avgpool2_hl(x)
    assert ops.saturation_raised()
    assert torch.equal(out, pool) and torch.equal(sp.hl, want) and sp.image == (2, H // 2, W // 2)
    none, sp2 = ops.avgpool2_hl(x, keep_f32=False)
    assert none is None and torch.equal(sp2.hl, want)
    ops.saturation_raised()
    _, sp3 = ops.avgpool2_hl(x.clamp(-10.0, 10.0))
    assert not ops.saturation_raised()
