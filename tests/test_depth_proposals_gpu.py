"""GPU: the depth proposals (csrc/pp_depth_proposals.hip, picopose_amd/depth_proposals.py) against tests/depth_proposals_oracle.py:
labels, plane scores, records and run lengths bit for bit, the refit plane against the float64 eigh fit of the same consensus set,
determinism across runs, streams and batch order, and depth_proposals / infer_depth_proposals end to end on the analytic scene."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_proposals_oracle as do  # noqa: E402
from netcfg import make_end_points, small_cfg  # noqa: E402

from picopose_amd import depth_proposals as dp  # noqa: E402

gpu = pytest.mark.gpu
REFIT_REL = 1e-9            # the bar tests/rgbd_pose_oracle.py holds the float64 Jacobi fits to
ZERO_PLANE = np.zeros(4, np.float32)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _range_labels(depths, cams, **kw):
    """The device's labels of a batch without planes: the range test alone decides the foreground."""
    B = len(depths)
    return dp.components(_cuda(np.stack(depths)), _cuda(np.stack(cams)), torch.zeros((B, 4), device="cuda"),
                         torch.zeros((B,), dtype=torch.int32, device="cuda"), **kw).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _frames(size):
    """(names, depths, the oracle's labels) of the label frames of one size; computed once and shared."""
    H, W = size
    fr = do.label_frames(H, W)
    want = [do.labels(d, do.foreground(d, do.camera(H, W), ZERO_PLANE, False)) for d in fr.values()]
    for w in want:
        w.setflags(write=False)
    return list(fr), list(fr.values()), want


@gpu
@pytest.mark.parametrize("size", do.LABEL_SIZES)
def test_labels_equal_the_oracle_bit_for_bit(size):
    """Serpentine, comb, checkerboard, full, empty, a component ending in the last pixel, steps exactly at and one float32 above
    max_step, zeros / NaNs / infinities: all frames of a size in ONE call (a batch of different images)."""
    names, depths, want = _frames(size)
    got = _range_labels(depths, [do.camera(*size)] * len(depths))
    assert got.dtype == np.int32 and got.shape == (len(depths),) + size
    for k, name in enumerate(names):
        n_comp = len(np.unique(want[k][want[k] >= 0]))
        print(f"{size} {name}: {n_comp} components, {int((want[k] >= 0).sum())} foreground pixels")
        assert np.array_equal(got[k], want[k]), name


@gpu
def test_labels_of_a_vga_frame_equal_the_oracle():
    d = do.big_frame()
    cam = do.camera(480, 640)
    want = do.labels(d, do.foreground(d, cam, ZERO_PLANE, False))
    got = _range_labels([d], [cam])[0]
    print(f"480x640: {len(np.unique(want[want >= 0]))} components")
    assert np.array_equal(got, want)


def _plane_scenes():
    a = do.table_scene(45, 70, do.E2E_RECTS, invalid=0.2, seed=1)
    b = do.table_scene(45, 70, ((5, 20, 40, 60, 90.0), (30, 40, 3, 30, 70.0)), normal=(-0.3, 0.2, -0.93), dist=650.0, invalid=0.2, seed=2)
    c = do.table_scene(45, 70, ((10, 30, 10, 50, 100.0),), normal=(0.0, -0.3, -0.95), dist=900.0, invalid=0.2, seed=3)
    return [a, b, c]


def _fit(depths, cams, **kw):
    out = dp.plane_fit(_cuda(np.stack(depths)), _cuda(np.stack(cams)), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_plane(got, b, want):
    info = got["info"][b]
    print(f"image {b}: winner {info[1]} (oracle {want['winner']}), count {info[2]} ({want['count']}), refit count {info[3]} ({want['refit_count']})")
    assert info.tolist() == [int(want["has_plane"]), want["winner"], want["count"], want["refit_count"]]
    p64, ref = got["plane64"][b], want["plane64"]
    if want["has_plane"]:
        err_n, err_d = np.abs(p64[:3] - ref[:3]).max(), abs(p64[3] - ref[3]) / abs(ref[3])
        print(f"   |n - eigh| = {err_n:.3e}, |d - eigh| / |d| = {err_d:.3e}  (bar {REFIT_REL:.0e})")
        assert err_n <= REFIT_REL and err_d <= REFIT_REL and p64[3] > 0
    else:
        assert not p64.any()
    assert np.array_equal(got["plane"][b].view(np.int32), p64.astype(np.float32).view(np.int32))     # the float32 plane is the cast


@gpu
@pytest.mark.parametrize("n_hyp", [64, 1024])
def test_plane_scores_winner_and_refit_equal_the_oracle(n_hyp):
    """Analytic tilted planes with raised rectangles and 20 % invalid pixels, three images in one call."""
    scenes = _plane_scenes()
    got = _fit([s[0] for s in scenes], [s[1] for s in scenes], n_hyp=n_hyp, seed=7, tau=5.0, min_inliers=500)
    for b, (depth, cam, _) in enumerate(scenes):
        _check_plane(got, b, do.plane(depth, cam, b, n_hyp, 7, 5.0, 500))


@gpu
def test_tied_hypotheses_keep_the_lower_index():
    depth, cam = do.roof_scene()
    want = do.plane(depth, cam, 0, 64, 0, 5.0, 100)
    top = np.flatnonzero(want["scores"] == want["count"])
    assert len(top) >= 2                                             # (tests/test_depth_proposals_cpu.py shows they lie on both planes)
    got = _fit([depth], [cam], n_hyp=64, seed=0, tau=5.0, min_inliers=100)
    assert got["info"][0, 1] == top[0]
    _check_plane(got, 0, want)


@gpu
def test_images_without_a_plane_fall_back_to_the_range_test():
    H, W = 45, 70
    cam = do.camera(H, W)
    dead = np.zeros((H, W), np.float32)
    dead[::2] = np.nan
    small, _, _ = do.table_scene(H, W, ((2, 40, 2, 60, 80.0),), invalid=0.2, seed=5)                 # the table is the smaller part
    normal, _, _ = do.table_scene(H, W, do.E2E_RECTS, invalid=0.2, seed=6)
    depths = [dead, small, normal]
    got = _fit(depths, [cam] * 3, n_hyp=128, seed=3, min_inliers=1700)
    want = [do.plane(d, cam, b, 128, 3, 5.0, 1700) for b, d in enumerate(depths)]
    # all invalid; the raised rectangle is the dominant plane and has enough inliers; the table of the third has too few
    assert [w["has_plane"] for w in want] == [False, True, False] and want[0]["count"] == 0 and want[2]["count"] >= 3
    for b in range(3):
        _check_plane(got, b, want[b])
    assert got["info"][0].tolist() == [0, 0, 0, 0]
    has = got["info"][:, 0].copy()
    lab = dp.components(_cuda(np.stack(depths)), _cuda(np.stack([cam] * 3)), _cuda(got["plane"]), _cuda(has), max_range=900.0).cpu().numpy()
    assert (lab[0] == -1).all()
    for b in range(3):
        assert np.array_equal(lab[b], do.labels(depths[b], do.foreground(depths[b], cam, got["plane"][b], bool(has[b]), max_range=900.0)))
    assert np.array_equal(lab[2], do.labels(depths[2], do.foreground(depths[2], cam, ZERO_PLANE, False, max_range=900.0))) and (lab[2] >= 0).any()


@gpu
def test_components_over_the_devices_own_plane_equal_the_oracle():
    """The oracle is fed the device's float32 plane, so this stage is bit-equal whatever the refit's last bits are."""
    scenes = _plane_scenes()
    depths, cams = [s[0] for s in scenes], [s[1] for s in scenes]
    got = _fit(depths, cams, n_hyp=64, seed=7, min_inliers=500)
    assert got["info"][:, 0].tolist() == [1, 1, 1]
    for kw in (dict(), dict(min_height=60.5, max_height=100.5, max_range=820.0, max_step=2.0)):
        lab = dp.components(_cuda(np.stack(depths)), _cuda(np.stack(cams)), _cuda(got["plane"]), _cuda(got["info"][:, 0].copy()), **kw).cpu().numpy()
        for b in range(3):
            okw = {k: v for k, v in kw.items() if k != "max_step"}
            want = do.labels(depths[b], do.foreground(depths[b], cams[b], got["plane"][b], True, **okw), kw.get("max_step", 15.0))
            print(f"image {b} {kw}: {len(np.unique(want[want >= 0]))} components")
            assert (want >= 0).any() and np.array_equal(lab[b], want)


def _records(n_q, recs, b):
    return sorted(tuple(int(v) for v in r) for r in recs[b, :min(int(n_q[b]), recs.shape[1])])


@gpu
def test_records_and_run_lengths_equal_the_oracle():
    names, depths, want_lab = _frames((96, 80))
    labels = _cuda(np.stack(want_lab))                               # (the oracle's labels: equal to the device's by the test above)
    B, H, W = labels.shape
    st = [do.stats(w) for w in want_lab]
    for min_area, max_area, drop in ((1, None, False), (3, 200, False), (1, None, True), (2, 5000, True)):
        n_q, recs = (t.cpu().numpy() for t in dp.component_stats(labels, min_area=min_area, max_area=max_area, drop_border=drop, cap=4096))
        for b in range(B):
            want = sorted(do.qualifying(st[b], min_area, H * W if max_area is None else max_area, drop))
            assert n_q[b] == len(want) and _records(n_q, recs, b) == want, (names[b], min_area, max_area, drop)
    # overflow at a small cap: the count says so, and what is written is a subset of the qualifiers
    n_q, recs = (t.cpu().numpy() for t in dp.component_stats(labels, cap=3))
    for b in range(B):
        want = do.qualifying(st[b], 1, H * W, False)
        got = _records(n_q, recs, b)
        assert n_q[b] == len(want) and len(got) == min(3, len(want)) and len(set(got)) == len(got) and set(got) <= set(want)
    # run lengths of every component of every frame (the checkerboard's 3840 single pixels among them)
    n_q, recs = (t.cpu().numpy() for t in dp.component_stats(labels, cap=4096))
    for b in range(B):
        if n_q[b] == 0:
            continue
        rows = dp.sort_records(recs[b, :n_q[b]], 4096)
        assert [tuple(r) for r in rows.tolist()] == do.qualifying(st[b], 1, H * W, False)           # area descending, then root
        sel = np.concatenate([np.full((len(rows), 1), b, np.int32), rows[:, [0, 2, 3, 4, 5]]], axis=1)
        table = dp.component_rle(labels, sel)
        ends, off_d, off, n_runs = table
        ends_h = ends.cpu().numpy()
        assert off[-1] == n_runs == len(ends_h) and np.array_equal(off_d.cpu().numpy(), off)
        for k, r in enumerate(rows):
            assert np.array_equal(ends_h[off[k]:off[k + 1]], do.run_ends(want_lab[b], int(r[0]))), (names[b], r.tolist())
        # the device's tables feed pp_rle_pack_bits as uploaded ones do: the packed areas are the records'
        bits, area = table.pack(H * W)
        assert np.array_equal(area.cpu().numpy(), rows[:, 1])


@gpu
def test_run_lengths_on_the_odd_frames():
    """45 x 70 (columns straddle mask words), 1 x 130 and 130 x 1: every component's run ends, from the device's own labels and boxes."""
    for size in ((45, 70), (1, 130), (130, 1)):
        names, depths, want_lab = _frames(size)
        labels = dp.components(_cuda(np.stack(depths)), _cuda(np.stack([do.camera(*size)] * len(depths))), torch.zeros((len(depths), 4), device="cuda"),
                               torch.zeros((len(depths),), dtype=torch.int32, device="cuda"))
        n_q, recs = (t.cpu().numpy() for t in dp.component_stats(labels, cap=4096))
        for b in range(len(depths)):
            st = do.stats(want_lab[b])
            assert _records(n_q, recs, b) == sorted(do.qualifying(st, 1, size[0] * size[1], False)), names[b]
            if n_q[b] == 0:
                continue
            rows = recs[b, :n_q[b]]
            sel = np.concatenate([np.full((len(rows), 1), b, np.int32), rows[:, [0, 2, 3, 4, 5]]], axis=1)
            ends, _, off, _ = dp.component_rle(labels, sel)
            ends = ends.cpu().numpy()
            for k, r in enumerate(rows):
                assert np.array_equal(ends[off[k]:off[k + 1]], do.run_ends(want_lab[b], int(r[0]))), (size, names[b], r.tolist())


def _e2e_batch():
    a, cam, _ = do.e2e_scene()
    b, _, _ = do.table_scene(45, 70, ((5, 20, 40, 60, 90.0), (30, 40, 3, 30, 70.0)), normal=(-0.3, 0.2, -0.93), dist=650.0, invalid=0.1, seed=2, keep_rects=True)
    c, _, _ = do.table_scene(45, 70, ((10, 30, 10, 50, 100.0),), normal=(0.0, -0.3, -0.95), dist=900.0)
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], np.float64)
    return [a, b, c], K


@gpu
def test_proposals_are_identical_across_runs_streams_and_batch_order():
    depths, K = _e2e_batch()
    kw = dict(min_inliers=500, min_area_px=50)
    first = dp.depth_proposals(np.stack(depths), K, **kw)
    assert [len(p) for p in first] == [5, 2, 1]
    assert dp.depth_proposals(np.stack(depths), K, **kw) == first
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert dp.depth_proposals(np.stack(depths), K, **kw) == first
    side.synchronize()
    assert dp.depth_proposals(np.stack(depths[::-1]), K, **kw) == first[::-1]
    for b in range(3):
        assert dp.depth_proposals(depths[b], K, **kw) == first[b]
    # uint16 depth goes through pp_depth_u16_scaled; the scene quantised to 0.1 mm keeps its rectangles
    raw = np.nan_to_num(np.rint(depths[0] * 10), nan=0.0).astype(np.uint16)
    assert [p["bbox"] for p in dp.depth_proposals(raw, K, depth_scale=0.1, **kw)] == [p["bbox"] for p in first[0]]


@pytest.fixture(scope="module")
def small_net():
    from picopose_amd.picopose import Net
    from picopose_amd.utils.seeding import seeded_state_dict

    net = Net(small_cfg())
    net.load_state_dict(seeded_state_dict(net.state_dict(), 5))
    return net.cuda().eval()


@gpu
def test_the_analytic_scene_end_to_end(small_net, monkeypatch):
    """A tilted plane and five rectangles raised 50-120 mm, two touching at different heights, one below min_area_px: the proposals are
    exactly the four large rectangles' masks, largest first (a condition, not a tolerance); label_proposals and inference take them."""
    from picopose_amd import ops
    from picopose_amd import proposals as pr
    from picopose_amd.pipeline import infer_depth_proposals

    monkeypatch.setattr(ops, "SATURATION_FLAG", False)          # plain seeded weights (tests/test_e2e.py's walk test explains)
    depth, cam, masks = do.e2e_scene()
    H, W = depth.shape
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], np.float64)
    props = dp.depth_proposals(depth, K, min_inliers=500)
    big = sorted((m for m in masks if m.sum() >= 200), key=lambda m: -int(m.sum()))
    assert len(props) == len(big) == 4
    for p, m in zip(props, big):
        ys, xs = np.nonzero(m)
        assert p["segmentation"] == do.rle_from_mask(m) and p["area"] == int(m.sum())
        assert p["bbox"] == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
    assert props == do.proposals(depth, cam, min_inliers=500)[0]

    net = small_net
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.clip(128 + 70 * np.sin(yy / 5.0)[..., None] * np.cos(xx / 7.0)[..., None] + rng.normal(0, 30, (H, W, 3)), 0, 255).astype(np.uint8)
    tem = {k: v.cuda() for k, v in make_end_points(2, 4, 71).items() if k.startswith("tem_")}
    tem["template_feature"] = torch.stack([net.precompute_templates(tem["tem_rgb"][o])["feature"] for o in range(2)])
    bank = pr.describe_templates(net, tem, [5, 9])
    records = pr.label_proposals(net, img, props, bank, scene_id=2, img_id=4, min_score=-1.0)
    assert len(records) >= 1 and all(any(r["segmentation"] is p["segmentation"] for p in props) for r in records)
    preds, data, dets, props2 = infer_depth_proposals(net, img, depth, K.ravel().tolist(), tem, bank, scene_id=2, img_id=4, min_score=-1.0, hyp=2, bs=2,
                                                      min_inliers=500)
    assert props2 == props and len(preds) == len(dets) == len(records) and data["score"].shape == (1, len(records), 1)
    assert [d["category_id"] for d in dets] == [r["category_id"] for r in records]
    assert all(len(h) == 2 and h[0]["R_stage_3"].shape == (9,) for h in preds)
    # with the RGB-D solver's radius the depth image is forwarded to inference as well
    preds, _, dets, _ = infer_depth_proposals(net, img, depth, K.ravel().tolist(), tem, bank, scene_id=2, img_id=4, min_score=-1.0, hyp=2, bs=2,
                                              min_inliers=500, rgbd_inlier_dist=0.01)
    assert len(preds) == len(dets) == len(records) and all("R_rgbd" in h[0] for h in preds)
