"""GPU: the proposal labelling (csrc/pp_proposals.hip, picopose_amd/proposals.py) against tests/proposal_oracle.py: pp_proposal_match
within err_bound(C) of the float64 statement with exact tie rules and position-independent bits, the mask kernels bit for bit, the
cls descriptors against torch's layer norm, and label_proposals / infer_proposals end to end on a small frame."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proposal_oracle as po  # noqa: E402
from netcfg import make_end_points, small_cfg  # noqa: E402

from picopose_amd import proposals as pr  # noqa: E402
from picopose_amd.masks import RunTable  # noqa: E402

gpu = pytest.mark.gpu


def _match(query, bank, T, topk):
    """-> (score, view, label, best) as numpy, and the device's unit bank rows."""
    b = pr.DescriptorBank.from_rows(torch.from_numpy(bank).cuda(), T, list(range(len(T))))
    out = pr.match_descriptors(torch.from_numpy(query).cuda(), b, topk)
    return [t.cpu().numpy() for t in out], b


def _check_against_oracle(query, bank, T, C, topk, planted=None):
    (score, view, label, best), _ = _match(query, bank, T, topk)
    m = po.match(query, bank, po.offsets_of(T), topk)
    bound = po.err_bound(C)
    P, O = len(query), len(T)
    assert score.shape == (P, O) and score.dtype == np.float32 and view.dtype == np.int32 and label.dtype == np.int32
    err = np.abs(score.astype(np.float64) - m["score"]).max()
    print(f"P={P} T={T} C={C} topk={topk} {'planted' if planted is not None else 'random'}: max |score - oracle| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.array_equal(best.view(np.int32), score[np.arange(P), label].view(np.int32))          # bit for bit
    assert (0 <= label).all() and (label < O).all() and (0 <= view).all() and (view < np.asarray(T)[None]).all()
    sure_l, sure_v = m["label_margin"] > 2 * bound, m["view_margin"] > 2 * bound
    assert np.array_equal(label[sure_l], m["label"][sure_l])
    assert np.array_equal(view[sure_v], m["view"][sure_v])
    if planted is not None:
        assert sure_l.all() and np.array_equal(label, planted)                                       # no case left out
    else:
        assert (~sure_l).sum() <= po.UNDECIDED_CAP * P and (~sure_v).sum() <= po.UNDECIDED_CAP * P * O


@gpu
@pytest.mark.parametrize("C", po.C_SET)
@pytest.mark.parametrize("T", po.T_SET)
@pytest.mark.parametrize("P", po.P_SET)
def test_proposal_match_is_within_the_bound_of_the_oracle(P, T, C):
    for topk in po.K_SET:
        query, bank, obj, _ = po.planted_set(P, T, C)
        _check_against_oracle(query, bank, T, C, topk, planted=obj)
        query, bank = po.random_set(P, T, C)
        _check_against_oracle(query, bank, T, C, topk)


@gpu
@pytest.mark.parametrize("C", [8, 384])
def test_ties_go_to_the_lowest_object_and_the_lowest_view(C):
    """Objects 0 and 2 hold the same rows, and rows 1 and 3 of that object are one row twice: every query planted on that row must be
    labelled 0 with view 1, and the twin objects' scores must be the same bits."""
    rng = np.random.default_rng(11)
    a = rng.standard_normal((5, C)).astype(np.float32)
    a[3] = a[1]
    other = rng.standard_normal((4, C)).astype(np.float32)
    bank = np.concatenate([a, other, a])
    query = (a[1][None] + 0.05 * rng.standard_normal((19, C))).astype(np.float32)
    for topk in (1, 5):
        (score, view, label, best), _ = _match(query, bank, (5, 4, 5), topk)
        assert np.array_equal(score[:, 0].view(np.int32), score[:, 2].view(np.int32))
        assert (label == 0).all() and (view[:, 0] == 1).all() and (view[:, 2] == 1).all()
        assert np.array_equal(best.view(np.int32), score[:, 0].view(np.int32))


@gpu
@pytest.mark.parametrize("C", [8, 384, 1024])
def test_scores_do_not_depend_on_the_position_of_the_proposal(C):
    T = (1, 4, 7)
    query, bank = po.random_set(19, T, C)
    first = query[:1]
    moved16 = np.concatenate([query[1:17], first, query[17:]])           # proposal 0 at position 16: the second tile's first slot
    moved17 = np.concatenate([query[1:18], first, query[18:]])           # ... and at position 17
    bits = lambda s, v, row: (s[row].view(np.int32).tolist(), v[row].tolist())  # noqa: E731
    for topk in (1, 5):
        want = None
        for q, row in ((first, 0), (query[:17], 0), (moved16, 16), (moved17, 17)):
            (score, view, _, _), _ = _match(np.ascontiguousarray(q), bank, T, topk)
            got = bits(score, view, row)
            want = got if want is None else want
            assert got == want


@gpu
@pytest.mark.parametrize("n", [1, 17, 40])
@pytest.mark.parametrize("size", [(5, 7), (48, 64)])
def test_mask_bits_and_intersections_equal_the_oracle(size, n):
    H, W = size
    segs = [po.rle_of(m) for m in po.mask_set(H, W, n)]
    runs = [np.cumsum(np.asarray(s["counts"], np.int64)) for s in segs]
    bits, area = RunTable.upload(runs, "cuda").pack(H * W)
    inter = pr.mask_intersections(bits)
    want_bits, want_area = po.pack_bits(segs)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), want_bits)
    assert np.array_equal(area.cpu().numpy(), want_area)
    assert np.array_equal(inter.cpu().numpy(), po.intersections(segs))
    inter2, area2 = pr.mask_overlaps(segs, (H, W))
    assert torch.equal(inter2, inter) and torch.equal(area2, area)


@pytest.fixture(scope="module")
def small_net():
    from picopose_amd.picopose import Net
    from picopose_amd.utils.seeding import seeded_state_dict

    net = Net(small_cfg())
    net.load_state_dict(seeded_state_dict(net.state_dict(), 5))
    return net.cuda().eval()


@gpu
def test_cls_descriptors_are_the_final_norm_of_the_cls_rows(small_net):
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(3)
    rgb = torch.randn(5, 3, 224, 224, generator=g).cuda()
    got = pr.cls_descriptors(small_net, rgb, bs=2)
    fe = small_net.feature_extractor
    with torch.no_grad():
        cls = torch.cat([fe.forward_tokens(rgb[s:s + 2].contiguous())[0][-1][:, 0] for s in range(0, 5, 2)]).cpu()
        want = F.layer_norm(cls, (384,), fe.dinov2.norm.weight.cpu(), fe.dinov2.norm.bias.cpu(), 1e-6)
    assert got.shape == (5, 384) and got.dtype == torch.float32
    err, scale = float((got.cpu() - want).abs().max()), max(1.0, float(want.abs().max()))
    print(f"max |cls descriptor - layer_norm| = {err:.3e} (scale {scale:.2f})")
    assert err <= 1e-5 * scale                                    # the bar of tests/test_engine_gpu.py's layer-norm test


@gpu
def test_label_proposals_equals_the_oracle_pipeline_and_feeds_inference(small_net, monkeypatch):
    from picopose_amd import ops
    from picopose_amd.pipeline import infer_proposals
    from picopose_amd.provider.test_batch import assemble_test_image

    monkeypatch.setattr(ops, "SATURATION_FLAG", False)          # plain seeded weights (tests/test_e2e.py's walk test explains)
    net = small_net
    H, W, obj_ids = 64, 96, [5, 9]
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.clip(128 + 70 * np.sin(yy / 5.0)[..., None] * np.cos(xx / 7.0)[..., None] + rng.normal(0, 30, (H, W, 3)), 0, 255).astype(np.uint8)
    masks = [np.zeros((H, W), np.uint8) for _ in range(3)]
    masks[0][8:40, 10:50] = 1                                    # a rectangle
    masks[1][8:40, 12:50] = 1                                    # an L that shares most of it
    masks[1][40:56, 12:28] = 1
    masks[2][30:60, 60:90] = 1                                   # a rectangle elsewhere
    proposals = [{"segmentation": po.rle_of(m)} for m in masks]
    tem = {k: v.cuda() for k, v in make_end_points(2, 4, 71).items() if k.startswith("tem_")}
    tem["template_feature"] = torch.stack([net.precompute_templates(tem["tem_rgb"][o])["feature"] for o in range(2)])
    bank = pr.describe_templates(net, tem, obj_ids)
    assert bank.rows.shape == (8, 384) and bank.offsets_host.tolist() == [0, 4, 8]
    norms = bank.rows.double().norm(dim=1).cpu().numpy()
    assert np.abs(norms - 1).max() < 1e-6
    sub = pr.describe_templates(net, tem, obj_ids, views=[3, 1])
    assert torch.allclose(sub.rows, bank.rows[[3, 1, 7, 5]], atol=1e-4)     # (another batch composition: not held to bits)

    # the device's own descriptors of the same crops, through the detection reader (same windows: the masks' boxes)
    K = [572.4114, 0.0, 48.0, 0.0, 573.57043, 32.0, 0.0, 0.0, 1.0]
    recs = [{"category_id": 5, "score": 1.0, "time": 0.0, "bbox": po.mask_box(m), "segmentation": p["segmentation"]} for m, p in zip(masks, proposals)]
    data = assemble_test_image(img, recs, K, {5: 0, 9: 1}, scene_id=2, img_id=4, rgb_mask_flag=True)
    desc = pr.cls_descriptors(net, data["real_rgb"][0]).cpu().numpy()
    unit = bank.rows.cpu().numpy()
    bound = po.err_bound(384)
    for kw in (dict(min_score=-1.0), dict(min_score=-1.0, max_detections=2), dict(min_score=-1.0, nms_iou=0.95), dict(min_score=2.0)):
        got = pr.label_proposals(net, img, proposals, bank, scene_id=2, img_id=4, time=0.5, **kw)
        want = po.label_pipeline(desc, unit, bank.offsets_host, obj_ids, [p["segmentation"] for p in proposals],
                                 **{"nms_iou": 0.25, "max_detections": 100, **kw})
        print(kw, [(r["category_id"], round(r["score"], 4), r["view"]) for r in got], want)
        assert len(got) == len(want)
        for r, (k, obj, score, view) in zip(got, want):
            assert r["segmentation"] is proposals[k]["segmentation"] and r["category_id"] == obj and r["view"] == view
            assert r["bbox"] == po.mask_box(masks[k]) and abs(r["score"] - score) <= bound
            assert (r["scene_id"], r["image_id"], r["time"]) == (2, 4, 0.5)
        assert [r["score"] for r in got] == sorted((r["score"] for r in got), reverse=True)
    assert pr.label_proposals(net, img, proposals, bank, scene_id=2, img_id=4, min_score=-1.0, min_area_px=10 ** 6) == []
    with pytest.raises(ValueError, match="proposal 1"):
        pr.label_proposals(net, img, [proposals[0], {"segmentation": {"size": [H, W], "counts": [3, 4]}}], bank, scene_id=2, img_id=4)

    records = pr.label_proposals(net, img, proposals, bank, scene_id=2, img_id=4, min_score=-1.0)
    preds, data2, dets = infer_proposals(net, img, proposals, K, tem, bank, scene_id=2, img_id=4, min_score=-1.0, hyp=2, bs=2)
    assert len(records) >= 1 and len(preds) == len(dets) == len(records) and data2["score"].shape == (1, len(records), 1)
    assert [d["category_id"] for d in dets] == [r["category_id"] for r in records]
    assert all(len(h) == 2 and h[0]["R_stage_3"].shape == (9,) for h in preds)
    assert infer_proposals(net, img, proposals, K, tem, bank, scene_id=2, img_id=4, min_score=2.0, hyp=2) == ([], None, [])
