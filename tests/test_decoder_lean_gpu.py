"""PP_DECODER_LEAN / PP_PATCH_OPERAND: the forward without the fp32 maps nothing reads (the render projection of every decoder level, the
finest DPT path map), without the torch glue around the flow's operand and with the patch-embed operand written from the image bank —
every output of every hypothesis bit for bit against the forward with the switches off; pp_flow_operand against the calls it replaces;
the pad channels the correlation lookup now writes itself."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from netcfg import make_end_points, small_cfg  # noqa: E402

from oracle.weights import seeded_state_dict  # noqa: E402

gpu = pytest.mark.gpu
B, N, HYP = 2, 6, 2


@pytest.fixture(scope="module")
def world():
    from picopose_amd import ops
    from picopose_amd.picopose import Net

    assert ops.PRECISION == "f16x3"
    net = Net(small_cfg())
    net.load_state_dict(seeded_state_dict(net.state_dict(), 23))
    net = net.cuda().eval()
    eps = []
    for seed in (71, 72):
        d = {k: v.cuda() for k, v in make_end_points(B, N, seed).items()}
        d["template_feature"] = torch.stack([net.feature_extractor(d["tem_rgb"][b])[-1] for b in range(B)])
        eps.append(d)
    yield net, eps
    ops.saturation_raised()             # (plain seeded decoders leave the operand range: DESIGN section 4)


def _clone(outs):
    return [{k: v.clone() for k, v in o.items()} for o in outs]


def _same(a, b):
    assert len(a) == len(b) == HYP
    for h in range(HYP):
        assert set(a[h]) == set(b[h])
        for k in a[h]:
            assert torch.equal(a[h][k], b[h][k]), (h, k)


def _runs(net, eps):
    """The forward without and with look-ahead crops, and the call that consumes the stash -> {name: outputs}."""
    net._query_stash = None
    out = {"plain": _clone(net(eps[0], HYP))}
    out["look-ahead"] = _clone(net(eps[0], HYP, next_real_rgb=eps[1]["real_rgb"]))
    assert net._query_stash is not None
    out["follow-up"] = _clone(net(eps[1], HYP))
    assert net._query_stash is None
    return out


@pytest.fixture(scope="module")
def reference(world):
    """Both switches off: what the forward computed before (computed once, shared)."""
    net, eps = world
    old = {k: os.environ.get(k) for k in ("PP_DECODER_LEAN", "PP_PATCH_OPERAND")}
    os.environ.update(PP_DECODER_LEAN="0", PP_PATCH_OPERAND="0")
    try:
        return _runs(net, eps)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@gpu
@pytest.mark.parametrize("lean,patch", [("1", "1"), ("1", "0"), ("0", "1")])
def test_every_output_keeps_its_bits(world, reference, monkeypatch, lean, patch):
    net, eps = world
    monkeypatch.setenv("PP_DECODER_LEAN", lean)
    monkeypatch.setenv("PP_PATCH_OPERAND", patch)
    got = _runs(net, eps)
    for name in reference:
        _same(got[name], reference[name])


@gpu
def test_the_switched_paths_are_the_ones_that_run(world, monkeypatch):
    """Defaults on: the decoder gets the finest path map as an operand only, the projection of the render maps stores no fp32 map, and the
    selected renders are never gathered; each switch restores its part."""
    from picopose_amd import ops

    net, eps = world
    seen = {"finest": [], "fr_out": [], "rgb_gathers": 0, "patch": 0}
    dec = net.offset_regressor.flow_decoder
    real_forward, real_conv, real_gather, real_patch = dec.forward_nhwc, ops.conv2d, ops.gather_rows, ops.patch_operand

    def forward_nhwc(tem, real, *a, **kw):
        seen["finest"].append((type(tem[-1]), type(real[-1])))
        return real_forward(tem, real, *a, **kw)

    def conv2d(x, wp, bias, ksize, *a, **kw):
        if kw.get("hl_into") is not None and kw["hl_into"][1] == 0 and ksize == 1:
            seen["fr_out"].append(kw.get("out") is not None)
        return real_conv(x, wp, bias, ksize, *a, **kw)

    def gather_rows(src, index):
        seen["rgb_gathers"] += tuple(src.shape[1:]) == (3, 224, 224)
        return real_gather(src, index)

    def patch_operand(*a, **kw):
        seen["patch"] += 1
        return real_patch(*a, **kw)

    monkeypatch.setattr(dec, "forward_nhwc", forward_nhwc)
    monkeypatch.setattr(ops, "conv2d", conv2d)
    monkeypatch.setattr(ops, "gather_rows", gather_rows)
    monkeypatch.setattr(ops, "patch_operand", patch_operand)
    monkeypatch.delenv("PP_DECODER_LEAN", raising=False)
    monkeypatch.delenv("PP_PATCH_OPERAND", raising=False)
    net(eps[0], HYP)
    assert seen == {"finest": [(ops.Split, ops.Split)], "fr_out": [False] * 3, "rgb_gathers": 0, "patch": 1}
    seen.update(finest=[], fr_out=[], rgb_gathers=0, patch=0)
    monkeypatch.setenv("PP_DECODER_LEAN", "0")
    monkeypatch.setenv("PP_PATCH_OPERAND", "0")
    net(eps[0], HYP)
    assert seen == {"finest": [(torch.Tensor, torch.Tensor)], "fr_out": [True] * 3, "rgb_gathers": 1, "patch": 0}


@gpu
@pytest.mark.parametrize("switch", ["PP_CORR_HL", "PP_CORR_TILED"])
def test_without_the_operand_lookup_the_fp32_projection_stays(world, monkeypatch, switch):
    """PP_CORR_HL=0 / PP_CORR_TILED=0: the lookup reads the fp32 render projection, which is therefore kept — the forward returns what it
    returned with the lean decoder switched off."""
    net, eps = world
    monkeypatch.setenv(switch, "0")
    monkeypatch.setenv("PP_DECODER_LEAN", "0")
    net._query_stash = None
    want = _clone(net(eps[0], HYP))
    monkeypatch.setenv("PP_DECODER_LEAN", "1")
    _same(_clone(net(eps[0], HYP)), want)


@gpu
def test_f16_mode_keeps_its_bits(world, monkeypatch):
    """The h-format engine: the lookup never takes the operand branch there (fp32 projection kept), the other lean parts apply."""
    from picopose_amd import ops

    net, eps = world
    with ops.precision_scope("f16"):
        ep = dict(eps[0])
        ep["template_feature"] = torch.stack([net.feature_extractor(ep["tem_rgb"][b])[-1] for b in range(B)])
        monkeypatch.setenv("PP_DECODER_LEAN", "0")
        monkeypatch.setenv("PP_PATCH_OPERAND", "0")
        net._query_stash = None
        want = _clone(net(ep, HYP))
        monkeypatch.setenv("PP_DECODER_LEAN", "1")
        monkeypatch.setenv("PP_PATCH_OPERAND", "1")
        _same(_clone(net(ep, HYP)), want)


@gpu
def test_dpt_head_nchw_drop_in_is_unchanged(world, monkeypatch):
    net, _ = world
    g = torch.Generator().manual_seed(9)
    feats = [torch.randn(2, 384, 16, 16, generator=g).cuda() for _ in range(4)]
    head = net.offset_regressor.dpt_head
    monkeypatch.setenv("PP_DECODER_LEAN", "0")
    want = [m.clone() for m in head(feats)]
    monkeypatch.setenv("PP_DECODER_LEAN", "1")
    got = head(feats)
    assert [tuple(m.shape) for m in got] == [(2, 256, 16, 16), (2, 256, 32, 32), (2, 256, 64, 64)]
    assert all(m.dtype == torch.float32 and torch.equal(m, w) for m, w in zip(got, want))


@gpu
@pytest.mark.parametrize("mode", ["f16x3", "f16"])
@pytest.mark.parametrize("Bf,H,W,ld", [(3, 16, 16, 2), (2, 64, 64, 2), (3, 16, 16, 8)])
def test_flow_operand_equals_the_calls_it_replaces(Bf, H, W, ld, mode):
    """zeros + slice assignment + split_activation -> one launch; the concat's flow columns patched from a strided view (no .contiguous())."""
    from picopose_amd import ops

    g = torch.Generator().manual_seed(11)
    wide = (torch.randn(Bf, H, W, ld, generator=g) * 20).cuda()
    flow = wide[..., 0:2]                                         # ld = 8: a view with pixel stride 8
    with ops.precision_scope(mode):
        flow8 = torch.zeros(Bf, H, W, 8, device="cuda")
        flow8[..., 0:2] = flow
        want = ops.split_activation(flow8, Bf, H * W, 8, H * W * 8, 8)
        sp = ops.flow_operand(flow)
        assert sp.image == (Bf, H, W) and torch.equal(sp.hl.view(torch.int16), want.view(torch.int16))
        cat = ops.Split.empty(Bf * H * W, 640, "cuda")
        cat.hl.copy_(torch.randn(cat.hl.shape, generator=g).half())
        ref = ops.Split(cat.hl.clone())
        ops.hl_patch_columns(flow.contiguous(), ref, 638)
        ops.hl_patch_columns(flow, cat, 638)
        assert torch.equal(cat.hl.view(torch.int16), ref.hl.view(torch.int16))
    assert not ops.saturation_raised()
    with ops.precision_scope(mode):                               # the saturation report of the split pass it replaces
        wide[0, 0, 1, 1] = -17000.0
        ops.flow_operand(wide[..., 0:2])
        assert ops.saturation_raised()


@gpu
@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("branch", ["operands", "PP_CORR_HL", "PP_CORR_TILED"])
def test_corr_lookup_writes_its_pad_channels(levels, branch, monkeypatch):
    """The result is allocated without a fill: the kernels write the zero pad channels (25 l -> a multiple of 8) themselves — exactly zero
    where the buffer held NaN, and the real channels are what the zero-filled allocation gave."""
    from picopose_amd import ops

    Bf, H, W, C, r = 2, 16, 16, 256, 2
    g = torch.Generator().manual_seed(13)
    f1, f2 = torch.randn(Bf, H, W, C, generator=g).cuda(), torch.randn(Bf, H, W, C, generator=g).cuda()
    flow = (torch.randn(Bf, H, W, 2, generator=g) * 3).cuda()
    flow[0, 0, 0] = 1.0e4                                          # a neighbourhood entirely outside the image
    n, pad = 25 * levels, -(-25 * levels // 8) * 8
    if branch != "operands":
        monkeypatch.setenv(branch, "0")
    hl = dict(f1_hl=(ops.split_image(f1), 0), f2_hl=ops.split_image(f2))
    assert ops.corr_takes_operands(hl["f1_hl"], hl["f2_hl"], H, W, C) == (branch == "operands")
    monkeypatch.setenv("PP_DECODER_LEAN", "0")
    want = ops.corr_lookup(f1, f2, flow, levels, r, c_pad=pad, **hl)
    monkeypatch.setenv("PP_DECODER_LEAN", "1")
    real_empty = torch.empty

    def nan_empty(*a, **kw):
        t = real_empty(*a, **kw)
        return t.fill_(float("nan")) if t.dtype == torch.float32 else t

    monkeypatch.setattr(torch, "empty", nan_empty)
    got = ops.corr_lookup(f1 if branch != "operands" else None, f2, flow, levels, r, c_pad=pad, **hl)
    monkeypatch.setattr(torch, "empty", real_empty)
    assert got.shape == (Bf, H, W, pad) and bool((got[..., n:] == 0).all())
    assert torch.equal(got[..., :n], want[..., :n]) and bool((want[..., n:] == 0).all())
