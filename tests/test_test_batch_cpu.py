"""CPU: the host side of the test-image assembly (picopose_amd/provider/test_batch.py) — COCO RLE parsing, pixel count and
extent from the runs, the crop windows, the score filter — and pp_detections_crop's argument validation through the ABI.

The RLE string vectors below come from a restatement of COCO's published rule (tests/detections_oracle.py), NOT from
pycocotools, which is not available: parity with pycocotools is unpinned."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detections_oracle as do  # noqa: E402

from oracle import preprocess as op  # noqa: E402
from picopose_amd.provider import test_batch as tb  # noqa: E402

VECTORS = [([3, 2, 4], "324", (3, 3)), ([3, 2, 4, 1], "324O", (2, 5)), ([20], "d0", (4, 5)), ([0, 5, 1000, 40, 3], "05Xo0S1kPO", (8, 131))]


def _masks():
    """>= 20 random blobs with 10 % holes plus the corner cases of the encoding."""
    rng = np.random.default_rng(3)
    out = [do.blob(rng, 480, 640) for _ in range(20)]
    m = do.blob(rng, 480, 640)
    m[0, 0] = 1                                              # leading 0-run empty
    out.append(m)
    m = np.zeros((480, 640), np.uint8)
    m[:, 100:103] = 1                                        # whole columns: one 1-run crosses columns
    m[200:, 99] = 1
    out.append(m)
    out.append(np.zeros((480, 640), np.uint8))               # all zero
    out.append(np.ones((1, 1), np.uint8))                    # 1 x 1 frames
    out.append(np.zeros((1, 1), np.uint8))
    out.append(np.ones((37, 53), np.uint8))                  # full frame
    out.append((rng.random((37, 53)) < 0.5).astype(np.uint8))
    return out


def _extent(mask):
    rows, cols = np.any(mask, axis=1), np.any(mask, axis=0)              # the expressions of get_bbox (data_utils.py:134-137)
    rmin, rmax = np.where(rows)[0][[0, -1]]
    cmin, cmax = np.where(cols)[0][[0, -1]]
    return int(rmin), int(rmax), int(cmin), int(cmax)


@pytest.mark.parametrize("counts,string,size", VECTORS)
def test_rle_string_vectors_both_directions(counts, string, size):
    assert do.counts_to_string(counts) == string and do.string_to_counts(string) == counts
    for form in (string, string.encode("ascii")):
        assert tb.rle_counts({"size": list(size), "counts": form}).tolist() == counts
    assert tb.rle_counts({"size": list(size), "counts": counts}).tolist() == counts


def test_rle_round_trip_count_extent_and_boxes():
    for k, m in enumerate(_masks()):
        h, w = m.shape
        counts = do.mask_to_counts_fast(m)
        if m.size <= 37 * 53:
            assert counts == do.mask_to_counts(m)
        if m[0, 0]:
            assert counts[0] == 0
        s = do.counts_to_string(counts)
        for form in (counts, s, s.encode("ascii")):
            seg = {"size": [h, w], "counts": form}
            got = tb.rle_counts(seg)
            assert got.dtype == np.int64 and got.tolist() == counts, k
            assert np.array_equal(do.decode(seg), m), k
        area, extent = tb.rle_area_extent(counts, h)
        assert area == int(m.sum()), k
        if area == 0:
            assert extent is None
            continue
        assert extent == _extent(m), k
        det = [3, 2, 5, 4]
        bbox, win = tb.detection_window(counts, (h, w), det)
        if area > 8:
            assert bbox == win == op.get_bbox(m), k
        else:
            assert bbox == det and win == op.get_square_bbox([2, 6, 3, 8], (h, w)), k


def test_windows_equal_the_reference_boxes(golden_dir):
    """tests/golden/preprocess_boxes.npz (outputs of the reference's get_bbox / get_square_bbox, incl. boxes clamped at every
    border): its masks encoded, masks drawn with its boxes' extents, and its boxes as detection boxes of the small-mask branch."""
    z = np.load(os.path.join(golden_dir, "preprocess_boxes.npz"))
    seen = 0
    for m, ratio, want in zip(z["masks"], z["mask_ratio"], z["mask_boxes"]):
        bbox, win = tb.detection_window(do.mask_to_counts(m), m.shape, [0, 0, 1, 1], minimum_n_point=0)
        assert bbox == win == op.get_bbox(m)
        if float(ratio) == 1.0:
            assert win == want.tolist()
            seen += 1
    assert seen >= 10
    clamped = set()
    for box, size, ratio, want in zip(z["boxes"], z["sizes"], z["box_ratio"], z["square_boxes"]):
        if float(ratio) != 1.0:
            continue
        r0, r1, c0, c1 = (int(v) for v in box)
        H, W = int(size[0]), int(size[1])
        tiny = np.zeros((H, W), np.uint8)
        tiny[H // 2, W // 2] = 1
        bbox, win = tb.detection_window(do.mask_to_counts_fast(tiny), (H, W), [c0, r0, c1 - c0, r1 - r0])
        assert bbox == [c0, r0, c1 - c0, r1 - r0] and win == want.tolist()
        if 0 <= r0 and r1 <= H and 0 <= c0 and c1 <= W:     # the same extent as a mask: two opposite corners are enough
            m = np.zeros((H, W), np.uint8)
            m[r0, c0] = m[r1 - 1, c1 - 1] = 1
            m[r0:r1, c0] = 1
            bbox, win = tb.detection_window(do.mask_to_counts_fast(m), (H, W), [0, 0, 1, 1], minimum_n_point=0)
            assert bbox == win == want.tolist() == op.get_bbox(m)
        wl = want.tolist()
        clamped |= {name for name, hit in (("top", wl[0] == 0), ("bottom", wl[1] == H), ("left", wl[2] == 0), ("right", wl[3] == W)) if hit}
    assert clamped == {"top", "bottom", "left", "right"}


def test_crop_affines_equal_the_per_instance_expressions():
    rng = np.random.default_rng(5)
    bboxes, windows = [], []
    for k in range(40):
        m = do.blob(rng, 480, 640)
        det = [int(v) for v in rng.integers(1, 200, 4)]
        if k % 5 == 0:
            m[:] = 0
            m[7, 9] = 1
        ref = op.crop_instance(np.zeros((480, 640, 3), np.uint8), m, det, img_size=28, pts_size=64)
        bbox, win = tb.detection_window(do.mask_to_counts_fast(m), (480, 640), det)
        assert bbox == ref["bbox"]
        bboxes.append(bbox)
        windows.append(win)
        M1, p1 = tb.crop_affines([bbox], [win], 224, 64)
        full = op.crop_instance(np.zeros((480, 640, 3), np.uint8), m, det) if k < 6 else None
        if full is not None:
            assert np.array_equal(M1[0], full["M"]) and np.array_equal(p1[0], full["pts2d"])
    M, pts = tb.crop_affines(bboxes, windows, 224, 64)
    for k in range(40):                                      # batched == one at a time
        M1, p1 = tb.crop_affines([bboxes[k]], [windows[k]], 224, 64)
        assert np.array_equal(M[k], M1[0]) and np.array_equal(pts[k], p1[0])


def test_filter_order_seg_time_and_none():
    m = np.zeros((30, 40), np.uint8)
    m[5:20, 8:30] = 1
    dets = [do.record(m, s, 1, time=t) for s, t in ((0.0, 1.5), (0.7, 0.1), (0.2, 0.2), (0.9, 0.3), (0.5, 0.4))]
    assert tb.select_detections(dets, 0.0) == ([1, 2, 3, 4], 1.5)        # given order, dets[0]['time'] before filtering
    assert tb.select_detections(dets, 0.5) == ([1, 3], 1.5)              # strictly above the filter score
    img = np.zeros((30, 40, 3), np.uint8)
    assert tb.assemble_test_image(img, dets, np.eye(3), {1: 0}, scene_id=1, img_id=2, seg_filter_score=0.95, device="cpu") is None
    assert do.collate(img, dets, np.eye(3), {1: 0}, 1, 2, seg_filter_score=0.95) is None
    ref = do.collate(img, dets, np.eye(3), {1: 0}, 1, 2, seg_filter_score=0.5, img_size=16, pts_size=4)
    assert ref["score"].shape == (1, 2, 1) and ref["score"][0, :, 0].tolist() == [np.float32(0.7), np.float32(0.9)]
    assert ref["seg_time"].tolist() == [[1.5]] and ref["real_rgb"].shape == (1, 2, 3, 16, 16) and ref["real_pts2d"].shape == (1, 2, 4, 4, 2)
    with pytest.raises(ValueError, match="no detections"):
        tb.select_detections([])


def test_malformed_rle_names_the_detection():
    m = np.zeros((30, 40), np.uint8)
    m[5:20, 8:30] = 1
    good = do.record(m, 0.9, 1)
    img = np.zeros((30, 40, 3), np.uint8)

    def bad(counts, size=(30, 40)):
        d = dict(good)
        d["segmentation"] = {"size": list(size), "counts": counts}
        return d

    s = good["segmentation"]["counts"]
    cases = [bad([100, 50]),                                  # sum != h * w
             bad([1300, -100]),                               # negative count
             bad(s[:-1] + chr(48 + ((ord(s[-1]) - 48) | 0x20))),   # truncated string: the last count announces another group
             bad(s + "1"),                                    # one run too many: sum != h * w
             bad([600, 600], size=(20, 60))]                  # a mask of another frame
    for c in cases:
        with pytest.raises(ValueError, match="detection 2"):
            tb.assemble_test_image(img, [good, dict(good, score=-1.0), c], np.eye(3), {1: 0}, scene_id=1, img_id=2, device="cpu")
    with pytest.raises(ValueError, match="detection 5"):
        tb.rle_counts({"size": [30, 40], "counts": [7]}, index=5)
    with pytest.raises(ValueError):
        tb.assemble_test_image(np.zeros((30, 40, 3), np.float32), [good], np.eye(3), {1: 0}, scene_id=1, img_id=2, device="cpu")


def test_pp_detections_crop_argument_validation_needs_no_gpu():
    from picopose_amd import _lib

    L = _lib.lib()
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    mean, std = (ctypes.c_double * 3)(0.5, 0.5, 0.5), (ctypes.c_double * 3)(0.2, 0.2, 0.2)
    i32 = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731

    def call(image=p, H=480, W=640, ends=p, n_runs=6, off=p, win=p, off_h=i32(0, 3, 6), win_h=i32(0, 100, 0, 100, 380, 480, 540, 640), n=2,
             S=224, mean3=mean, std3=std, rgb=p, mask=p):
        return L.pp_detections_crop(image, H, W, ends, n_runs, off, win, off_h, win_h, n, S, 0, mean3, std3, rgb, mask, None)

    for kw in ({"image": None}, {"ends": None}, {"off": None}, {"win": None}, {"off_h": None}, {"win_h": None}, {"mean3": None},
               {"std3": None}, {"rgb": None}, {"mask": None},
               {"n": 0}, {"n": -1}, {"n": 70000}, {"S": 0}, {"S": -224}, {"H": 0}, {"W": -1}, {"H": 50000, "W": 50000}, {"n_runs": 0},
               {"off_h": i32(0, 4, 3)},                                    # run_offset decreases
               {"off_h": i32(-1, 3, 6)}, {"off_h": i32(0, 3, 7)},          # negative / past n_runs
               {"win_h": i32(0, 100, 0, 100, 380, 481, 540, 640)},         # below the frame
               {"win_h": i32(0, 100, 0, 100, 380, 480, 540, 641)},         # right of the frame
               {"win_h": i32(-1, 100, 0, 100, 380, 480, 540, 640)}, {"win_h": i32(0, 100, -2, 100, 380, 480, 540, 640)},
               {"win_h": i32(50, 50, 0, 100, 380, 480, 540, 640)},         # empty rows
               {"win_h": i32(0, 100, 30, 20, 380, 480, 540, 640)}):        # empty columns
        assert call(**kw) == -1, kw
