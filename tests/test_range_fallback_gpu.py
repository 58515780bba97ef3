"""GPU: the evaluator's exact-mode fallback (pipeline.py on_saturation="exact") — a mini-batch whose forward clamped an f16x3 operand is
re-run in strict fp32 and returns poses instead of raising; the stream-ordered snapshot (pp_saturation_take) that tells the mini-batches
apart; the per-model arithmetic mode (Net.precision) it runs on."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from netcfg import make_end_points, small_cfg  # noqa: E402
from test_e2e import _load_cal, _vit_cfg  # noqa: E402

from oracle.weights import seeded_state_dict  # noqa: E402

gpu = pytest.mark.gpu


def _same_preds(a, b):
    """Two infer_batch / infer_image results bit for bit (NaN = NaN)."""
    assert len(a) == len(b)
    for ha, hb in zip(a, b):
        assert len(ha) == len(hb)
        for x, y in zip(ha, hb):
            for k in x:
                if k == "pnp_success":
                    assert x[k] == y[k]
                else:
                    assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True), k


def _as_image_preds(batch_preds):
    """infer_batch's hypotheses in infer_image's form (run_test.py:181-186)."""
    return [[{"R_stage_3": np.asarray(h["R"]).reshape(9), "t_stage_3": np.asarray(h["t"]).reshape(3) * 1000,
              "inliers_ratio": h["inliers_ratio"]} for h in hyps] for hyps in batch_preds]


def _outlier_net(golden_dir, factor):
    """The calibrated ViT-B network with 4 channels of every ls1 / ls2.gamma times `factor` (tests/test_e2e.py, outlier test)."""
    from picopose_amd.picopose import Net

    tag = "vitb_b2n6"
    z, B, N, hyp, seed, vit, ref, weights = _load_cal(golden_dir, tag)
    net = Net(_vit_cfg(vit))
    sd = weights(net.state_dict())
    g = torch.Generator().manual_seed(1234)
    for k in sd:
        if k.endswith(("ls1.gamma", "ls2.gamma")):
            ch = torch.randperm(sd[k].numel(), generator=g)[:4]
            sd[k] = sd[k].clone()
            sd[k][ch] *= factor
    net.load_state_dict(sd)
    net = net.cuda().eval()
    dev = {k: v.cuda() for k, v in make_end_points(B, N, seed, tem_pose=torch.from_numpy(z[f"{tag}/tem_pose_all"]), dome=True).items()}
    with torch.no_grad():
        dev["template_feature"] = torch.stack([net.feature_extractor(dev["tem_rgb"][b])[-1] for b in range(B)])
    return net, dev, hyp


@gpu
@pytest.mark.parametrize("factor", [300.0, 3000.0])
def test_outlier_channels_fall_back_to_exact_mode_instead_of_raising(golden_dir, factor):
    """The residual-channel spread of a trained DINOv2 makes the default f16x3 forward clamp an operand (test_e2e.py: the 1x1 layer behind
    the lookup); with on_saturation="exact" the batch is recomputed in strict fp32 and its poses are the f32 network's, bit for bit."""
    from picopose_amd import _lib, ops
    from picopose_amd.pipeline import infer_batch

    net, dev, hyp = _outlier_net(golden_dir, factor)
    assert ops.PRECISION == "f16x3" and not ops.saturation_raised()
    got = infer_batch(net, dev, hyp, on_saturation="exact")
    assert net.range_fallbacks == 1
    assert ops.PRECISION == "f16x3" and net.precision is None and net.match_mode is None
    assert not ops.saturation_raised()
    net.precision, net.match_mode = "f32", "exact"
    want = infer_batch(net, dev, hyp)
    net.precision, net.match_mode = None, None
    _same_preds(got, want)
    assert ops.PRECISION == "f16x3" and not ops.saturation_raised()
    with pytest.raises(_lib.PicoPoseHipError, match="saturated"):          # the default is still the error
        infer_batch(net, dev, hyp)
    assert net.range_fallbacks == 1 and not ops.saturation_raised()         # (the error path reset the word)


@gpu
def test_infer_image_reruns_only_the_mini_batch_that_clamped(golden_dir):
    """Three mini-batches, pipelined (mini-batch j + 1 launched before mini-batch j's poses are read): only the middle one's crops leave the
    operand range.  Its snapshot alone is set — mini-batches 0 and 2 keep the f16x3 poses, mini-batch 1 gets the f32 poses, one re-run.
    (The live word read with mini-batch 0's poses would already hold mini-batch 1's clamp.)"""
    from picopose_amd import _lib, ops
    from picopose_amd.picopose import Net
    from picopose_amd.pipeline import infer_batch, infer_image

    tag = "vitb_b2n6"
    z, _, N, hyp, seed, vit, ref, weights = _load_cal(golden_dir, tag)
    net = Net(_vit_cfg(vit))
    net.load_state_dict(weights(net.state_dict()))
    net = net.cuda().eval()
    n, bs = 6, 2
    ep = {k: v.cuda() for k, v in make_end_points(n, N, seed + 100, dome=True).items()}
    ep["real_rgb"][2:4] *= 1.0e4                     # |4 x| far beyond 65504 in the middle mini-batch's crops
    with torch.no_grad():
        ep["template_feature"] = torch.stack([net.feature_extractor(ep["tem_rgb"][o])[-1] for o in range(n)])   # one object per instance
    tem = {k: v for k, v in ep.items() if k.startswith("tem_") or k == "template_feature"}
    data = {k: v[None] for k, v in ep.items() if k.startswith("real_")}
    data["obj_idx"] = torch.arange(n, device="cuda")[None]
    data["score"] = torch.ones(1, n, device="cuda")
    inputs = lambda a, b: dict({k: v[a:b].contiguous() for k, v in ep.items() if k.startswith("real_")},  # noqa: E731
                               **{k: v[a:b].contiguous() for k, v in tem.items()})

    assert not ops.saturation_raised()
    got = infer_image(net, data, tem, hyp=hyp, bs=bs, on_saturation="exact")
    assert net.range_fallbacks == 1 and ops.PRECISION == "f16x3" and net.precision is None
    assert not ops.saturation_raised()
    assert len(got) == n
    for b in (0, 2):
        _same_preds(got[b * bs:(b + 1) * bs], _as_image_preds(infer_batch(net, inputs(b * bs, (b + 1) * bs), hyp)))
    assert not ops.saturation_raised()
    net.precision, net.match_mode = "f32", "exact"
    _same_preds(got[2:4], _as_image_preds(infer_batch(net, inputs(2, 4), hyp)))
    net.precision, net.match_mode = None, None
    with pytest.raises(_lib.PicoPoseHipError, match="saturated"):           # the middle mini-batch alone, default mode: the error
        infer_batch(net, inputs(2, 4), hyp)
    # the sequential walk makes the same choice
    _same_preds(infer_image(net, data, tem, hyp=hyp, bs=bs, pipelined=False, on_saturation="exact"), got)
    assert net.range_fallbacks == 2 and not ops.saturation_raised()


@gpu
def test_two_models_in_different_modes_interleave_like_each_alone():
    """Net.precision is the model's, not the process's: an f32 and an f16x3 model called alternately return what each returns alone
    under the global mode, whatever the global says meanwhile."""
    from picopose_amd import ops
    from picopose_amd.picopose import Net

    nets = []
    for seed in (3, 4):
        net = Net(small_cfg())
        net.load_state_dict(seeded_state_dict(net.state_dict(), seed))
        nets.append(net.cuda().eval())
    ep = {k: v.cuda() for k, v in make_end_points(2, 4, 81).items()}
    with torch.no_grad():
        ep["template_feature"] = torch.stack([nets[0].feature_extractor(ep["tem_rgb"][b])[-1] for b in range(2)])
    hyp, modes, old = 2, ("f32", "f16x3"), ops.PRECISION
    try:
        alone = []
        for net, mode in zip(nets, modes):
            ops.PRECISION = mode
            alone.append([{k: v.clone() for k, v in o.items()} for o in net(ep, hyp)])
        ops.PRECISION = "f16"                       # a third mode as the global: neither model follows it
        for net, mode in zip(nets, modes):
            net.precision = mode
        for _ in range(2):
            for net, want in zip(nets, alone):
                got = net(ep, hyp)
                for h in range(hyp):
                    for k in want[h]:
                        assert torch.equal(got[h][k], want[h][k]), (net.precision, h, k)
        assert ops.PRECISION == "f16" and ops.precision() == "f16"
    finally:
        ops.PRECISION = old
        ops.saturation_raised()                     # (plain seeded decoders leave the operand range: DESIGN section 4)


@gpu
def test_saturation_take_on_a_side_stream():
    """pp_saturation_take in stream order: a producer's flag and a host-side fill enqueued before it land in the slot and the word is left
    clear; a clear word gives 0; null pointers are rejected."""
    from picopose_amd import _lib, ops

    w = ops.saturation_word()
    assert w is not None
    ops.saturation_raised()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    big = torch.zeros(64, 64, device="cuda")
    big[5, 7] = 3.0e4                               # 4 x > 65504: the split pass clamps and flags
    slot_hit, slot_clear, slot_fill = (torch.full((1,), 7, dtype=torch.int32, device="cuda") for _ in range(3))
    with torch.cuda.stream(side), torch.no_grad():
        ops.split_activation(big, 1, 64, 64, 0, 64)
        ops.saturation_take(big.device, slot_hit)
        ops.saturation_take(big.device, slot_clear)
        w.fill_(1)
        ops.saturation_take(big.device, slot_fill)
    side.synchronize()
    assert int(slot_hit.item()) == 1 and int(slot_clear.item()) == 0 and int(slot_fill.item()) == 1
    assert int(w.item()) == 0
    L = _lib.lib()
    sp = torch.cuda.current_stream().cuda_stream
    assert L.pp_saturation_take(None, slot_hit.data_ptr(), sp) == -1
    assert L.pp_saturation_take(w.data_ptr(), None, sp) == -1
    assert L.pp_saturation_take(None, None, sp) == -1
    torch.cuda.synchronize()
    assert int(slot_hit.item()) == 1 and int(w.item()) == 0          # (nothing was launched by the rejected calls)
