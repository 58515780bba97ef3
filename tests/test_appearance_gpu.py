"""GPU: the appearance score (csrc/pp_appearance.hip, picopose_amd/proposals.py) against tests/appearance_oracle.py:
pp_appearance_match within its float64 bounds with the exact lowest-index rule and position-independent bits, pp_patch_valid bit for
bit, token_descriptors against torch's layer norm, and label_proposals(appearance=True) / infer_proposals end to end on a small frame."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import appearance_oracle as ao  # noqa: E402
import proposal_oracle as po  # noqa: E402
from netcfg import make_end_points, small_cfg  # noqa: E402

from picopose_amd import proposals as pr  # noqa: E402

gpu = pytest.mark.gpu


def _bank(bank, t_valid):
    """A DescriptorBank of R one-view objects whose patch rows are `bank` (R, N, C) raw, normalised on the device."""
    R, _, C = bank.shape
    return pr.DescriptorBank.from_rows(torch.ones(R, C).cuda(), [1] * R, list(range(R)), torch.from_numpy(bank).cuda(),
                                       torch.from_numpy(t_valid).cuda())


def _run(query, q_valid, bank, t_valid, rows):
    """-> (app, patch_sim, patch_arg, n_valid) as numpy."""
    out = pr.appearance_scores(torch.from_numpy(query).cuda(), torch.from_numpy(q_valid).cuda(), _bank(bank, t_valid), rows)
    return [t.cpu().numpy() for t in out]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@gpu
@pytest.mark.parametrize("C", ao.C_SET)
@pytest.mark.parametrize("N", ao.N_SET)
def test_appearance_match_is_within_the_bounds_of_the_oracle(N, C):
    for P in ao.P_SET:
        for pattern in ao.PATTERNS:
            query, q_valid, bank, t_valid, rows = ao.random_case(P, N, C, pattern)
            app, sim, arg, n_valid = _run(query, q_valid, bank, t_valid, rows)
            m = ao.appearance(query, q_valid, bank, t_valid, rows)
            assert sim.shape == (P, N) and sim.dtype == np.float32 and arg.dtype == np.int32 and n_valid.dtype == np.int32
            assert app.shape == (P,) and app.dtype == np.float32
            e_sim = np.abs(sim.astype(np.float64) - m["patch_sim"]).max()
            e_app = np.abs(app.astype(np.float64) - m["app"])
            b_app = np.array([ao.app_bound(C, max(int(n), 1)) for n in m["n_valid"]])
            print(f"P={P} N={N} C={C} {pattern}: max |patch_sim - oracle| = {e_sim:.3e} (bound {ao.sim_bound(C):.3e}), "
                  f"max |app - oracle| = {e_app.max():.3e} (bound {b_app.min():.3e})")
            assert e_sim <= ao.sim_bound(C) and (e_app <= b_app).all()
            assert np.array_equal(n_valid, m["n_valid"])
            sure = m["margin"] > 2 * ao.e_cos(C)
            assert np.array_equal(arg[sure], m["patch_arg"][sure])
            assert (~sure).sum() <= ao.UNDECIDED_CAP * P * N
            if pattern == "no_template":
                assert (_bits(sim) == 0).all() and (arg == -1).all() and (_bits(app) == 0).all()
            else:
                assert (arg >= 0).all() and (arg < N).all() and t_valid[rows[:, None], arg].all()      # only valid template patches
            if pattern == "no_query":
                assert (n_valid == 0).all() and (_bits(app) == 0).all()


@gpu
@pytest.mark.parametrize("C", ao.PLANTED_C)
@pytest.mark.parametrize("N", ao.PLANTED_N)
def test_planted_patches_are_found(N, C):
    for P in (3, 5):
        query, q_valid, bank, t_valid, rows, perm = ao.planted_case(P, N, C)
        app, sim, arg, n_valid = _run(query, q_valid, bank, t_valid, rows)
        assert np.array_equal(arg, perm)                         # everywhere: no case is left out
        assert (app > 0.9).all() and np.array_equal(n_valid, q_valid.sum(1))
        m = ao.appearance(query, q_valid, bank, t_valid, rows)
        b_app = np.array([ao.app_bound(C, int(n)) for n in m["n_valid"]])       # (_half leaves no proposal without a valid patch)
        assert (np.abs(app - m["app"]) <= b_app).all() and np.abs(sim - m["patch_sim"]).max() <= ao.sim_bound(C)


@gpu
@pytest.mark.parametrize("C", [8, 384])
@pytest.mark.parametrize("N", [16, 300])
def test_ties_go_to_the_lowest_patch_and_twin_views_give_the_same_bits(N, C):
    """Template patches 3 and 7 hold the same row (the other lane half; with N = 300 also patch 70, another wave, and patch 280, the
    second chunk of 256 patches), views 0 and 2 hold the same rows: every query planted on that row reports 3, and the twin views
    give the same bits."""
    rng = np.random.default_rng(11)
    bank = rng.standard_normal((3, N, C)).astype(np.float32)
    bank[0, 7] = bank[0, 3]
    if N > 280:
        bank[0, 70] = bank[0, 280] = bank[0, 3]
    bank[2] = bank[0]
    t_valid = np.ones((3, N), np.uint8)
    t_valid[:, 1] = 0
    query = np.tile(bank[0, 3][None, None] + 0.05 * rng.standard_normal((1, 1, C)), (2, N, 1)).astype(np.float32)
    query[:, 1] = bank[0, 1]                                     # planted on an invalid template patch: it must not be reported
    q_valid = np.ones((2, N), np.uint8)
    app, sim, arg, _ = _run(query, q_valid, bank, t_valid, np.int32([0, 2]))
    planted = np.arange(N) != 1
    assert (arg[:, planted] == 3).all() and (arg[:, 1] != 1).all()
    assert np.array_equal(_bits(sim[0]), _bits(sim[1])) and _bits(app)[0] == _bits(app)[1] and np.array_equal(arg[0], arg[1])
    assert (_bits(sim[:, planted]) == _bits(sim[:, 0:1])).all()               # equal query rows: equal bits in every tile and lane


@gpu
@pytest.mark.parametrize("C", [8, 384, 1024])
def test_scores_do_not_depend_on_the_position_of_the_proposal(C):
    """One proposal alone, first of 5 and last of 5 (another workgroup index, other neighbours), and the same rows at another patch
    position (another tile and lane)."""
    N = 130                                                      # three query tiles, the last one part-filled
    query, q_valid, bank, t_valid, _ = ao.random_case(5, N, C, "half")
    one, v_one = query[:1], q_valid[:1]
    want = None
    for q, v, rows, at in ((one, v_one, [1], 0), (query, q_valid, [1, 0, 3, 2, 1], 0),
                           (np.concatenate([query[1:], one]), np.concatenate([q_valid[1:], v_one]), [0, 3, 2, 1, 1], 4),
                           (np.concatenate([query[1:3], one]), np.concatenate([q_valid[1:3], v_one]), [3, 3, 1], 2)):
        app, sim, arg, n_valid = _run(np.ascontiguousarray(q), np.ascontiguousarray(v), bank, t_valid, np.int32(rows))
        got = (_bits(sim[at]).tolist(), arg[at].tolist(), int(_bits(app)[at]), int(n_valid[at]))
        want = got if want is None else want
        assert got == want
    # the patches rolled by 70 places: every row lands in another tile and lane, its cosines keep their bits
    roll = np.roll(one, 70, axis=1)
    _, sim_r, arg_r, _ = _run(np.ascontiguousarray(roll), np.roll(v_one, 70, axis=1), bank, t_valid, np.int32([1]))
    assert np.roll(_bits(sim_r[0]), -70).tolist() == want[0] and np.roll(arg_r[0], -70).tolist() == want[1]


@gpu
@pytest.mark.parametrize("S", [28, 224])
def test_patch_valid_equals_the_oracle(S):
    rng = np.random.default_rng([7, S])
    n = 6
    mask = (rng.random((n, S, S)) < rng.choice([0.3, 0.5, 0.7], (n, 1, 1))).astype(np.float32)
    mask[0] = 0.0
    mask[0, :7, :14] = 1.0                                       # exactly half of patch 0
    mask[0, 14:21, 14:28] = 1.0                                  # ... and one pixel short in patch (1, 1)
    mask[0, 14, 14] = 0.0
    mask[1] *= rng.random((S, S)).astype(np.float32) * 2         # soft values on both sides of 0.5
    mask[2, ::3] = np.nan
    mask[3] = 1.0
    valid, n_valid = pr.patch_valid(torch.from_numpy(mask).cuda(), 14)
    want, want_n = ao.patch_valid(mask, 14)
    assert valid.dtype == torch.uint8 and n_valid.dtype == torch.int32 and valid.shape == (n, (S // 14) ** 2)
    assert np.array_equal(valid.cpu().numpy(), want) and np.array_equal(n_valid.cpu().numpy(), want_n)
    assert want[0, 0] == 1 and want[0, S // 14 + 1] == 0 and want_n[0] == 1 and want_n[3] == (S // 14) ** 2


@pytest.fixture(scope="module")
def small_net():
    from picopose_amd.picopose import Net
    from picopose_amd.utils.seeding import seeded_state_dict

    net = Net(small_cfg())
    net.load_state_dict(seeded_state_dict(net.state_dict(), 5))
    return net.cuda().eval()


@gpu
def test_token_descriptors_are_the_final_norm_of_the_token_rows(small_net):
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(3)
    rgb = torch.randn(5, 3, 224, 224, generator=g).cuda()
    cls, patches = pr.token_descriptors(small_net, rgb, bs=2)
    fe = small_net.feature_extractor
    with torch.no_grad():
        tok = torch.cat([fe.forward_tokens(rgb[s:s + 2].contiguous())[0][-1] for s in range(0, 5, 2)]).cpu()
        want = F.layer_norm(tok, (384,), fe.dinov2.norm.weight.cpu(), fe.dinov2.norm.bias.cpu(), 1e-6)
    assert cls.shape == (5, 384) and patches.shape == (5, 256, 384) and patches.dtype == torch.float32 and patches.is_contiguous()
    err, scale = float((patches.cpu() - want[:, 1:]).abs().max()), max(1.0, float(want.abs().max()))
    print(f"max |patch tokens - layer_norm| = {err:.3e} (scale {scale:.2f})")
    assert err <= 1e-5 * scale                                    # the bar of the cls test in tests/test_proposals_gpu.py
    assert torch.equal(cls, pr.cls_descriptors(small_net, rgb, bs=2))       # bit for bit, for the same bs
    empty = pr.token_descriptors(small_net, rgb[:0])
    assert empty[0].shape == (0, 384) and empty[1].shape == (0, 256, 384)


@gpu
def test_label_proposals_with_appearance_equals_the_oracle_pipeline_and_feeds_inference(small_net, monkeypatch):
    from picopose_amd import ops
    from picopose_amd.pipeline import infer_proposals
    from picopose_amd.provider.test_batch import assemble_test_image

    monkeypatch.setattr(ops, "SATURATION_FLAG", False)          # plain seeded weights, as in tests/test_proposals_gpu.py
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
    plain = pr.describe_templates(net, tem, obj_ids)
    bank = pr.describe_templates(net, tem, obj_ids, patches=True)
    assert plain.patch_rows is None and torch.equal(bank.rows, plain.rows) and bank.offsets_host.tolist() == [0, 4, 8]
    assert bank.patch_rows.shape == (8, 256, 384) and bank.patch_valid.shape == (8, 256) and bank.patch_valid.dtype == torch.uint8
    assert np.abs(bank.patch_rows.double().norm(dim=2).cpu().numpy() - 1).max() < 1e-6
    assert np.array_equal(bank.patch_valid.cpu().numpy(), ao.patch_valid(tem["tem_mask"].reshape(8, 224, 224).cpu().numpy(), 14)[0])
    sub = pr.describe_templates(net, tem, obj_ids, views=[3, 1], patches=True)
    assert torch.equal(sub.patch_valid, bank.patch_valid[[3, 1, 7, 5]])
    assert torch.allclose(sub.patch_rows, bank.patch_rows[[3, 1, 7, 5]], atol=1e-4)      # (another batch composition: not held to bits)
    with pytest.raises(ValueError, match="patches=True"):
        pr.label_proposals(net, img, proposals, plain, scene_id=2, img_id=4, appearance=True)

    # the device's own descriptors, patch tokens and crop masks of the same crops, through the detection reader
    K = [572.4114, 0.0, 48.0, 0.0, 573.57043, 32.0, 0.0, 0.0, 1.0]
    recs = [{"category_id": 5, "score": 1.0, "time": 0.0, "bbox": po.mask_box(m), "segmentation": p["segmentation"]} for m, p in zip(masks, proposals)]
    data = assemble_test_image(img, recs, K, {5: 0, 9: 1}, scene_id=2, img_id=4, rgb_mask_flag=True)
    desc, tokens = (t.cpu().numpy() for t in pr.token_descriptors(net, data["real_rgb"][0]))
    q_valid, n_q = ao.patch_valid(data["real_mask"][0].cpu().numpy(), 14)
    assert (n_q > 0).all()
    unit, patch_unit, patch_ok = bank.rows.cpu().numpy(), bank.patch_rows.cpu().numpy(), bank.patch_valid.cpu().numpy()
    segs = [p["segmentation"] for p in proposals]
    for kw in (dict(min_score=-1.0), dict(min_score=-1.0, max_detections=2), dict(min_score=-1.0, nms_iou=0.95),
               dict(min_score=-1.0, appearance_weight=3.0), dict(min_score=-1.0, appearance_weight=0.0), dict(min_score=2.0)):
        w = kw.get("appearance_weight", 1.0)
        got = pr.label_proposals(net, img, proposals, bank, scene_id=2, img_id=4, time=0.5, appearance=True, **kw)
        okw = {"nms_iou": 0.25, "max_detections": 100, **kw}
        okw.pop("appearance_weight", None)
        want = ao.label_pipeline(desc, unit, bank.offsets_host, obj_ids, segs, tokens, q_valid, patch_unit, patch_ok, weight=w, **okw)
        print(kw, [(r["category_id"], round(r["score"], 4), round(r["semantic_score"], 4), round(r["appearance_score"], 4), r["view"]) for r in got], want)
        assert len(got) == len(want)
        b_sem = po.err_bound(384)
        for r, (k, obj, score, view, sem, app) in zip(got, want):
            b_app = ao.app_bound(384, int(n_q[k]))               # the proposal's own count of valid patches
            assert r["segmentation"] is proposals[k]["segmentation"] and r["category_id"] == obj and r["view"] == view
            assert r["bbox"] == po.mask_box(masks[k]) and (r["scene_id"], r["image_id"], r["time"]) == (2, 4, 0.5)
            assert abs(r["semantic_score"] - sem) <= b_sem and abs(r["appearance_score"] - app) <= b_app
            assert abs(r["score"] - score) <= (b_sem + w * b_app) / (1 + w)
            assert r["score"] == float(ao.combine(np.float32(r["semantic_score"]), np.float32(r["appearance_score"]), w))
        assert [r["score"] for r in got] == sorted((r["score"] for r in got), reverse=True)

    # against the call without appearance: the same semantic score, label and view per proposal, bit for bit; no new key there
    base = pr.label_proposals(net, img, proposals, bank, scene_id=2, img_id=4, min_score=-1.0, nms_iou=1.0)
    full = pr.label_proposals(net, img, proposals, bank, scene_id=2, img_id=4, min_score=-1.0, nms_iou=1.0, appearance=True)
    assert len(base) == len(full) == 3
    by_seg = {id(r["segmentation"]): r for r in base}
    for r in full:
        b = by_seg[id(r["segmentation"])]
        assert r["semantic_score"] == b["score"] and r["category_id"] == b["category_id"] and r["view"] == b["view"] and r["bbox"] == b["bbox"]
        assert 0.0 < r["appearance_score"] <= 1.0 + ao.sim_bound(384)
    keys = {"scene_id", "image_id", "category_id", "bbox", "score", "time", "segmentation", "view"}
    assert all(set(r) == keys for r in base) and all(set(r) == keys | {"semantic_score", "appearance_score"} for r in full)
    assert base == pr.label_proposals(net, img, proposals, plain, scene_id=2, img_id=4, min_score=-1.0, nms_iou=1.0)
    timings = {}
    pr.label_proposals(net, img, proposals, bank, scene_id=2, img_id=4, min_score=-1.0, appearance=True, timings=timings)
    assert set(timings) == {"host", "crop", "vit", "match", "appearance", "overlaps"} and timings["appearance"] > 0

    records = pr.label_proposals(net, img, proposals, bank, scene_id=2, img_id=4, min_score=-1.0, appearance=True)
    preds, data2, dets = infer_proposals(net, img, proposals, K, tem, bank, scene_id=2, img_id=4, min_score=-1.0, hyp=2, bs=2, appearance=True)
    assert len(records) >= 1 and len(preds) == len(dets) == len(records) and data2["score"].shape == (1, len(records), 1)
    assert [(d["category_id"], d["score"], d["appearance_score"]) for d in dets] == [(r["category_id"], r["score"], r["appearance_score"]) for r in records]
    assert all(len(h) == 2 and h[0]["R_stage_3"].shape == (9,) for h in preds)
