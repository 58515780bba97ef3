"""GPU: picopose_amd.provider.test_batch.assemble_test_image (csrc/pp_detect.hip) — one launch for an image's detections, masks
read from their run lengths — bit for bit against the existing per-detection helper utils.preprocess.crop_instance on the
decoded masks, and against the CPU statement of the whole call (tests/detections_oracle.py) with test_preprocess.py's bar for
the colours (|rgb - oracle| <= 1e-6, double arithmetic on both sides).  pycocotools and cv2 are not available: both sides
restate their published definitions."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detections_oracle as do  # noqa: E402
from netcfg import make_end_points, small_cfg  # noqa: E402

from picopose_amd.provider import test_batch as tb  # noqa: E402
from picopose_amd.utils import preprocess as hp  # noqa: E402

gpu = pytest.mark.gpu
KEYS_EQUAL = ("score", "obj_id", "obj_idx", "real_pts2d", "real_bbox", "real_mask", "real_M", "real_K", "real_pose", "scene_id", "img_id",
              "seg_time")


def _by_hand(img, dets, K, obj_idxs, scene_id, img_id, flag, seg_filter_score=0.0):
    """The loop the call replaces: decode each RLE to a frame-sized mask, crop_instance per kept detection, collate."""
    kept = [d for d in dets if d["score"] > seg_filter_score]
    rows = [hp.crop_instance(img, do.decode(d["segmentation"]), d["bbox"], rgb_mask_flag=flag) for d in kept]
    dev = rows[0]["rgb"].device
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)  # noqa: E731
    i32 = lambda a: torch.from_numpy(np.asarray(a, np.int32)).to(dev)  # noqa: E731
    n = len(rows)
    return {"score": f32([[d["score"]] for d in kept])[None], "obj_id": i32([[d["category_id"]] for d in kept])[None],
            "obj_idx": i32([[obj_idxs[d["category_id"]]] for d in kept])[None],
            "real_pts2d": torch.stack([r["pts2d"].float() for r in rows]).to(dev)[None],
            "real_rgb": torch.stack([r["rgb"] for r in rows])[None], "real_bbox": f32([r["bbox"] for r in rows])[None],
            "real_mask": torch.stack([r["mask"] for r in rows])[None], "real_M": torch.stack([r["M"] for r in rows]).to(dev)[None],
            "real_K": f32(np.array(K, np.float64).reshape(3, 3))[None].repeat(n, 1, 1)[None],
            "real_pose": torch.eye(4, device=dev)[None].repeat(n, 1, 1)[None],
            "scene_id": i32([[scene_id]]), "img_id": i32([[img_id]]), "seg_time": f32([[dets[0]["time"]]])}


def _check(img, dets, K, obj_idxs, flag, n_kept):
    got = tb.assemble_test_image(img, dets, K, obj_idxs, scene_id=3, img_id=11, rgb_mask_flag=flag)
    hand = _by_hand(img, dets, K, obj_idxs, 3, 11, flag)
    ref = do.collate(img, dets, K, obj_idxs, 3, 11, rgb_mask_flag=flag)
    assert got["score"].shape == (1, n_kept, 1) and set(got) == set(hand) == set(ref)
    for k in hand:                                            # bit-equal to the per-detection helper, the colours included
        assert got[k].dtype == hand[k].dtype and got[k].shape == hand[k].shape, k
        assert torch.equal(got[k], hand[k]), k
    for k in KEYS_EQUAL:
        assert got[k].cpu().numpy().dtype == ref[k].dtype and np.array_equal(got[k].cpu().numpy(), ref[k]), k
    err = np.abs(got["real_rgb"].cpu().numpy() - ref["real_rgb"]).max()
    print(f"max |rgb - oracle| = {err:.3e}")
    assert err <= 1e-6
    return got


@gpu
@pytest.mark.parametrize("n", [1, 8, 33])
@pytest.mark.parametrize("frame", [(480, 640), (960, 1280), (37, 53)])
@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("seed", [0, 1])
def test_assembled_image_equals_crop_instance_and_the_oracle(seed, flag, frame, n):
    img, dets, K, obj_idxs = do.scene(seed, frame[0], frame[1], n)
    assert len(dets) == n + 1                                 # one record at the filter score is dropped
    _check(img, dets, K, obj_idxs, flag, n)


@gpu
@pytest.mark.parametrize("flag", [False, True])
def test_masks_with_more_runs_than_the_lds_slice_take_the_global_path(flag):
    """A checkerboard region: every column of it holds ~120-240 runs, so the ends that touch one tile's source columns exceed
    the 2048 the workgroup stages and it searches global memory instead; a smooth blob in the same image stays staged."""
    H, W = 480, 640
    img, dets, K, obj_idxs = do.scene(5, H, W, 2)
    yy, xx = np.mgrid[0:H, 0:W]
    board = np.zeros((H, W), np.uint8)
    board[20:460, 100:560] = ((yy + xx) & 1)[20:460, 100:560]
    stripes = np.zeros((H, W), np.uint8)
    stripes[0:480, 0:640] = (yy & 1)
    dets = dets + [do.record(board, 0.6, 1), do.record(stripes, 0.55, 3)]
    counts = tb.rle_counts(dets[-2]["segmentation"])
    assert len(counts) > 100 * 2048 // 16                     # far beyond the slice for any tile of this crop
    _check(img, dets, K, obj_idxs, flag, 4)


@gpu
def test_list_and_string_records_give_identical_tensors():
    a = do.scene(2, 480, 640, 8, compressed=True)
    b = do.scene(2, 480, 640, 8, compressed=False)
    assert isinstance(a[1][0]["segmentation"]["counts"], str) and isinstance(b[1][0]["segmentation"]["counts"], list)
    byt = [dict(d, segmentation=dict(d["segmentation"], counts=d["segmentation"]["counts"].encode("ascii"))) for d in a[1]]
    x = tb.assemble_test_image(*a, scene_id=1, img_id=2)
    for dets in (b[1], byt):
        y = tb.assemble_test_image(a[0], dets, a[2], a[3], scene_id=1, img_id=2)
        assert all(torch.equal(x[k], y[k]) for k in x)


@gpu
def test_grey_and_rgba_images():
    img, dets, K, obj_idxs = do.scene(4, 120, 160, 3)
    grey = np.ascontiguousarray(img[..., 0])
    x = tb.assemble_test_image(grey, dets, K, obj_idxs, scene_id=1, img_id=2)
    y = tb.assemble_test_image(np.stack([grey] * 3, axis=2), dets, K, obj_idxs, scene_id=1, img_id=2)
    rgba = np.concatenate([img, np.full(img.shape[:2] + (1,), 77, np.uint8)], axis=2)
    z = tb.assemble_test_image(rgba, dets, K, obj_idxs, scene_id=1, img_id=2)
    w = tb.assemble_test_image(img, dets, K, obj_idxs, scene_id=1, img_id=2)
    assert all(torch.equal(x[k], y[k]) and torch.equal(z[k], w[k]) for k in x)


@gpu
def test_call_enqueues_on_a_side_stream_without_a_host_wait():
    img, dets, K, obj_idxs = do.scene(6, 480, 640, 8)
    ref = tb.assemble_test_image(img, dets, K, obj_idxs, scene_id=1, img_id=2, rgb_mask_flag=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    # a long-running kernel queue in front on the side stream: a call that waited for its stream would return after it
    blocker = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(40):
            blocker = blocker @ blocker * 1e-3
        done = torch.cuda.Event()
    got = tb.assemble_test_image(img, dets, K, obj_idxs, scene_id=1, img_id=2, rgb_mask_flag=True, stream=side)
    with torch.cuda.stream(side):
        done.record()
    returned_early = not done.query()
    side.synchronize()
    assert all(torch.equal(got[k], ref[k]) for k in ref)
    assert torch.cuda.current_stream() != side
    print("call returned before its stream drained:", returned_early)
    assert returned_early


@gpu
def test_infer_image_on_the_assembled_data_equals_the_hand_collated_data(monkeypatch):
    from picopose_amd import ops
    from picopose_amd.picopose import Net
    from picopose_amd.pipeline import infer_detections, infer_image
    from picopose_amd.utils.seeding import seeded_state_dict

    monkeypatch.setattr(ops, "SATURATION_FLAG", False)       # plain seeded weights (tests/test_e2e.py's walk test explains)
    net = Net(small_cfg())
    net.load_state_dict(seeded_state_dict(net.state_dict(), 5))
    net = net.cuda().eval()
    n_obj, N, hyp = 3, 4, 2
    tem = {k: v.cuda() for k, v in make_end_points(n_obj, N, 71).items() if k.startswith("tem_")}
    tem["template_feature"] = torch.stack([net.precompute_templates(tem["tem_rgb"][o])["feature"] for o in range(n_obj)])
    img, dets, K, obj_idxs = do.scene(7, 480, 640, 5)
    hand = _by_hand(img, dets, K, obj_idxs, 3, 11, False)
    want = infer_image(net, hand, tem, hyp=hyp, bs=2)
    preds, data = infer_detections(net, img, dets, K, tem, obj_idxs, scene_id=3, img_id=11, hyp=hyp, bs=2)
    assert all(torch.equal(data[k], hand[k]) for k in hand)
    assert len(preds) == len(want) == 5
    for ha, hb in zip(preds, want):
        for x, y in zip(ha, hb):
            assert np.array_equal(x["R_stage_3"], y["R_stage_3"]) and np.array_equal(x["t_stage_3"], y["t_stage_3"])
            assert np.array_equal(np.asarray(x["inliers_ratio"]), np.asarray(y["inliers_ratio"]))
    assert infer_detections(net, img, dets, K, tem, obj_idxs, scene_id=3, img_id=11, seg_filter_score=0.99, hyp=hyp) == ([], None)
