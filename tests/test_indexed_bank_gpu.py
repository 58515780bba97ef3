"""GPU: the indexed template bank — stage 1 on per-object banks (pp_stage1_*_indexed), Net.forward with end_points["template_index"]
and pipeline.infer_image(indexed_bank=True) — gives bit for bit what the gathered bank bank[obj_index] gives, without the copy."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from netcfg import make_end_points, small_cfg  # noqa: E402

from oracle.weights import seeded_state_dict  # noqa: E402

gpu = pytest.mark.gpu


def _pattern(name, B):
    """-> (O, obj_index (B,) int64): crops of distinct / one / mixed objects, unsorted, objects no crop uses, O = 1."""
    g = torch.Generator().manual_seed(B)
    if name == "distinct":
        O = B + 3
        return O, torch.randperm(O, generator=g)[:B]
    if name == "one":
        return 3, torch.full((B,), 1, dtype=torch.int64)
    if name == "mixed":
        return 6, torch.randint(0, 4, (B,), generator=g)          # objects 4, 5 unused
    if name == "unsorted":
        return 4, (torch.arange(B) * 3 + 2) % 4
    return 1, torch.zeros(B, dtype=torch.int64)                  # "single": a bank of one object


def _bank(O, N, C, seed, dtype):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(O, N, C, 16, 16, device="cuda", generator=g).to(dtype)


def _query(B, C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, C, 16, 16, device="cuda", generator=g)
    yy, xx = torch.meshgrid(torch.arange(224.0), torch.arange(224.0), indexing="ij")
    m = (((yy - 111.5) ** 2 + (xx - 111.5) ** 2) < (0.4 * 224) ** 2).float()[None].repeat(B, 1, 1).cuda()
    return q, m


def _same_stage1(bank, idx, query, mask, mode, topk=5):
    from picopose_amd.utils import matching as hm

    gathered = bank[idx.to(bank.device)]
    s_i, i_i = hm.matching_templates_indexed(bank, idx, query, None, mask, topk=topk, mode=mode)
    s_g, i_g = hm.matching_templates(gathered, query, None, mask, topk=topk, mode=mode)
    a_i, st_i = hm.template_scores_indexed(bank, idx, query, mask, mode=mode, return_stats=True)
    a_g, st_g = hm.template_scores(gathered, query, mask, mode=mode, return_stats=True)
    assert torch.equal(i_i, i_g) and torch.equal(s_i, s_g)
    assert torch.equal(a_i, a_g)
    assert torch.equal(st_i, st_g), (st_i.tolist(), st_g.tolist())
    return st_i


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_indexed_stage1_equals_gathered_bank(mode, dtype):
    """(32, 162, 768): the 8-wave shape, full rounds of the striped walk; every index pattern; the index on the device and on the host."""
    B, N, C = 32, 162, 768
    query, mask = _query(B, C, 5)
    for k, name in enumerate(("distinct", "one", "mixed", "unsorted", "single")):
        O, idx = _pattern(name, B)
        bank = _bank(O, N, C, 100 + k, dtype)
        _same_stage1(bank, idx.cuda(), query, mask, mode)
        if name == "mixed":
            _same_stage1(bank, idx, query, mask, mode)               # a CPU index: range-checked, copied without blocking
        del bank


@gpu
@pytest.mark.parametrize("waves", ["4", "8"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_indexed_stage1_small_shapes_and_chunks(mode, dtype, waves, monkeypatch):
    """Fewer than two items per CU (the 4-wave shape on template halves), both workgroup shapes pinned, several chunk sizes of
    an object's crops (PP_S1_CPX: placement only) — and a grid that is not a multiple of 8 (no striping)."""
    monkeypatch.setenv("PP_S1_WAVES", waves)
    for B, N, C in ((6, 20, 384), (13, 7, 64)):
        query, mask = _query(B, C, B)
        for name in ("one", "mixed", "distinct", "single"):
            O, idx = _pattern(name, B)
            bank = _bank(O, N, C, 7 * B + N, dtype)
            for cpx in ("1", "3", "64"):
                monkeypatch.setenv("PP_S1_CPX", cpx)
                _same_stage1(bank, idx.cuda(), query, mask, mode)
            monkeypatch.delenv("PP_S1_CPX")


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_indexed_stage1_near_ties_reevaluated_like_gathered(dtype):
    """Duplicated templates, a query equal to a template and planted near-ties with patch 0: the fast mode's exact re-evaluation runs
    (stats nonzero) on the rows of the crop's object, and gives what it gives on the gathered bank."""
    B, N, C, O = 6, 12, 384, 3
    idx = torch.tensor([2, 0, 2, 2, 1, 0], device="cuda")
    g = torch.Generator().manual_seed(78)
    bank = torch.randn(O, N, C, 256, generator=g)
    bank[:, 7] = bank[:, 3]                                       # duplicated templates
    for s in (5, 40, 200):                                        # template patches near copies of patch 0 (row decisions)
        bank[:, :, :, s] = bank[:, :, :, 0] * (1.0 + 2e-5 * torch.randn(O, N, C, generator=g))
    query = torch.randn(B, C, 256, generator=g)
    query[1] = bank[0, 4]                                         # a query equal to a template of its object
    for t in (7, 130):                                            # query patches near copies of patch 0 (column decisions)
        query[:, :, t] = query[:, :, 0] * (1.0 + 2e-5 * torch.randn(B, C, generator=g))
    mask = torch.ones(B, 224, 224)
    bank = bank.reshape(O, N, C, 16, 16).cuda().to(dtype)
    query = query.reshape(B, C, 16, 16).cuda()
    st = _same_stage1(bank, idx, query, mask.cuda(), "fast").tolist()
    assert st[0] + st[1] > 0 and st[2] > 0, st


def _net(seed, batched=True, precision=None):
    from picopose_amd.picopose import Net

    net = Net(small_cfg())
    net.load_state_dict(seeded_state_dict(net.state_dict(), seed))
    net = net.cuda().eval()
    net.batch_hypotheses = batched
    net.precision = precision
    return net


def _same_outputs(got, ref):
    assert len(got) == len(ref)
    for h in range(len(ref)):
        assert set(got[h]) == set(ref[h])
        for k in ref[h]:
            assert torch.equal(got[h][k], ref[h][k]), (h, k)


@gpu
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("cache", [False, True])
@pytest.mark.parametrize("batched", [True, False])
def test_forward_with_template_index_equals_gathered_forward(batched, cache, precision):
    net = _net(21, batched, precision)
    O, N, hyp = 3, 5, 3
    idx = torch.tensor([2, 0, 2, 1], device="cuda")
    tem = {k: v.cuda() for k, v in make_end_points(O, N, 33).items() if k.startswith("tem_")}
    real = {k: v.cuda() for k, v in make_end_points(len(idx), 1, 34).items() if k.startswith("real_")}
    banks = [net.precompute_templates(tem["tem_rgb"][o], chunk=3) for o in range(O)]
    tem["template_feature"] = torch.stack([b["feature"] for b in banks])
    gathered = dict(real, **{k: v[idx].contiguous() for k, v in tem.items()})
    indexed = dict(real, **tem, template_index=idx)
    if cache:
        dpt = [torch.stack([b["dpt"][k] for b in banks]) for k in range(3)]
        gathered["template_cache"] = {"obj_index": idx, "dpt": dpt}
        indexed["template_cache"] = {"obj_index": idx.clone(), "dpt": dpt}    # (another tensor with the same objects)
    _same_outputs(net(indexed, hyp), net(gathered, hyp))


@gpu
def test_forward_rejects_inconsistent_template_index():
    net = _net(21)
    O, N, hyp = 3, 5, 2
    idx = torch.tensor([2, 0], device="cuda")
    tem = {k: v.cuda() for k, v in make_end_points(O, N, 33).items() if k.startswith("tem_")}
    real = {k: v.cuda() for k, v in make_end_points(2, 1, 34).items() if k.startswith("real_")}
    tem["template_feature"] = torch.stack([net.feature_extractor(tem["tem_rgb"][o])[-1] for o in range(O)])
    ep = dict(real, **tem, template_index=idx)
    with pytest.raises(ValueError):                                   # the bank tensors disagree on O
        net(dict(ep, tem_rgb=tem["tem_rgb"][:2]), hyp)
    with pytest.raises(ValueError):
        net(dict(ep, template_feature=tem["template_feature"][:, :4]), hyp)
    with pytest.raises(ValueError):                                   # wrong dtype / length of the index
        net(dict(ep, template_index=idx.int()), hyp)
    with pytest.raises(ValueError):
        net(dict(ep, template_index=idx[:1]), hyp)
    banks = [net.precompute_templates(tem["tem_rgb"][o], chunk=3) for o in range(O)]
    dpt = [torch.stack([b["dpt"][k] for b in banks]) for k in range(3)]
    with pytest.raises(ValueError):                                   # template_cache names other objects
        net(dict(ep, template_cache={"obj_index": torch.tensor([2, 1], device="cuda"), "dpt": dpt}), hyp)


def _same_preds(a, b):
    assert len(a) == len(b)
    for ha, hb in zip(a, b):
        assert len(ha) == len(hb)
        for x, y in zip(ha, hb):
            assert np.array_equal(x["R_stage_3"], y["R_stage_3"]) and np.array_equal(x["t_stage_3"], y["t_stage_3"])
            assert np.array_equal(np.asarray(x["inliers_ratio"]), np.asarray(y["inliers_ratio"]))


def _image(net, n_obj, N, obj_idx, seed):
    tem = {k: v.cuda() for k, v in make_end_points(n_obj, N, seed).items() if k.startswith("tem_")}
    banks = [net.precompute_templates(tem["tem_rgb"][o]) for o in range(n_obj)]
    tem["template_feature"] = torch.stack([b["feature"] for b in banks])
    inst = {k: v.cuda() for k, v in make_end_points(len(obj_idx), 1, seed + 1).items() if k.startswith("real_")}
    data = {k: v[None] for k, v in inst.items()}
    data["obj_idx"] = torch.tensor([obj_idx], device="cuda")
    data["score"] = torch.linspace(0.9, 0.5, len(obj_idx), device="cuda")[None]
    return tem, banks, data


@gpu
def test_infer_image_indexed_bank_equals_default(monkeypatch):
    """infer_image(..., indexed_bank=True): pipelined and sequential walks, next_data, the extended bank — the default call's poses."""
    from picopose_amd import ops
    from picopose_amd.pipeline import infer_image

    monkeypatch.setattr(ops, "SATURATION_FLAG", False)       # (plain seeded weights: test_e2e.py's walk test explains)
    net = _net(5)
    hyp = 2
    tem, banks, data = _image(net, 3, 4, [1, 0, 1, 1, 2], 71)
    _, _, data2 = _image(net, 3, 4, [2, 2], 91)
    for pipelined in (True, False):
        _same_preds(infer_image(net, data, tem, hyp=hyp, bs=2, pipelined=pipelined, indexed_bank=True),
                    infer_image(net, data, tem, hyp=hyp, bs=2, pipelined=pipelined))
    plain1, plain2 = infer_image(net, data, tem, hyp=hyp, bs=2), infer_image(net, data2, tem, hyp=hyp, bs=2)
    ahead1 = infer_image(net, data, tem, hyp=hyp, bs=2, next_data=data2, indexed_bank=True)
    assert net._query_stash is not None
    ahead2 = infer_image(net, data2, tem, hyp=hyp, bs=2, indexed_bank=True)
    assert net._query_stash is None
    _same_preds(ahead1, plain1)
    _same_preds(ahead2, plain2)
    tem["template_cache"] = {"dpt": [torch.stack([b["dpt"][k] for b in banks]) for k in range(3)]}
    for pipelined in (True, False):
        _same_preds(infer_image(net, data, tem, hyp=hyp, bs=2, pipelined=pipelined, indexed_bank=True),
                    infer_image(net, data, tem, hyp=hyp, bs=2, pipelined=pipelined))


@gpu
def test_infer_image_indexed_bank_exact_rerun():
    """on_saturation="exact": the plain seeded decoder leaves the f16x3 operand range, so mini-batches are re-run in strict fp32 —
    with the same indexed inputs, the same poses and the same number of re-runs as the default call."""
    from picopose_amd.pipeline import infer_image

    net = _net(5)
    tem, _, data = _image(net, 2, 4, [1, 0, 1], 72)
    for pipelined in (True, False):
        before = net.range_fallbacks
        got = infer_image(net, data, tem, hyp=2, bs=2, pipelined=pipelined, on_saturation="exact", indexed_bank=True)
        reruns = net.range_fallbacks - before
        want = infer_image(net, data, tem, hyp=2, bs=2, pipelined=pipelined, on_saturation="exact")
        assert net.range_fallbacks - before - reruns == reruns
        _same_preds(got, want)


@gpu
def test_infer_image_indexed_bank_peak_memory(monkeypatch):
    """ViT-S, N = 64, 8 detections of 2 objects: without the per-detection copy of the bank, the peak allocation drops by at least
    0.9 x (B - O) x one object's template bytes."""
    from picopose_amd import ops
    from picopose_amd.pipeline import infer_image

    monkeypatch.setattr(ops, "SATURATION_FLAG", False)
    net = _net(5)
    n_obj, N, B = 2, 64, 8
    tem = {k: v.cuda() for k, v in make_end_points(n_obj, N, 81).items() if k.startswith("tem_")}
    with torch.no_grad():
        tem["template_feature"] = torch.stack([net.feature_extractor(tem["tem_rgb"][o])[-1] for o in range(n_obj)])
    inst = {k: v.cuda() for k, v in make_end_points(B, 1, 82).items() if k.startswith("real_")}
    data = {k: v[None] for k, v in inst.items()}
    data["obj_idx"] = torch.tensor([[0, 1, 1, 0, 1, 1, 0, 1]], device="cuda")
    data["score"] = torch.ones(1, B, device="cuda")
    obj_bytes = sum(v[0].numel() * v.element_size() for v in tem.values())

    def peak(indexed):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        preds = infer_image(net, data, tem, hyp=3, bs=16, indexed_bank=indexed)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, preds

    peak(False), peak(True)                                        # warm: workspaces, packed weights, the allocator's pools
    gathered, p_g = peak(False)
    indexed, p_i = peak(True)
    _same_preds(p_i, p_g)
    assert gathered - indexed >= 0.9 * (B - n_obj) * obj_bytes, (gathered, indexed, obj_bytes)
