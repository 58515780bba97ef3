"""CPU: the proposal labelling's argument checks (no device is touched before they return), the host NMS against the brute-force
oracle, the oracle itself on the planted and random sets the GPU tests use, and the record format."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proposal_oracle as po  # noqa: E402

from picopose_amd import _lib  # noqa: E402

EINVAL = -1


def _host_ptr(nbytes=256, misalign=0):
    buf = (ctypes.c_char * (nbytes + 32))()
    p = ctypes.addressof(buf)
    return buf, p + (-p) % 16 + misalign


def _offsets(*v):
    return (ctypes.c_int * len(v))(*v)


def test_match_rejects_bad_arguments_without_a_device():
    L = _lib.lib()
    keep, p = _host_ptr()
    ok_off = _offsets(0, 2, 3)
    good = dict(query=p, P=4, bank=p, offsets=p, offsets_host=ok_off, O=2, C=8, topk=5, score=p, view=p, label=p, best=p)
    order = ("query", "P", "bank", "offsets", "offsets_host", "O", "C", "topk", "score", "view", "label", "best")
    call = lambda **kw: L.pp_proposal_match(*[{**good, **kw}[k] for k in order], None)  # noqa: E731
    for name in ("query", "bank", "offsets", "offsets_host", "score", "view", "label", "best"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("P", "O", "C"):
        for bad in (0, -1):
            assert call(**{name: bad}) == EINVAL, (name, bad)
    assert call(C=6) == EINVAL                                   # not a multiple of 4
    assert call(C=1028) == EINVAL                                # beyond the LDS staging (PP_MATCH_MAX_C = 1024)
    assert call(topk=0) == EINVAL and call(topk=9) == EINVAL
    assert call(offsets_host=_offsets(1, 2, 3)) == EINVAL        # does not start at 0
    assert call(offsets_host=_offsets(0, 3, 2)) == EINVAL        # decreases
    assert call(offsets_host=_offsets(0, 0, 3)) == EINVAL        # object 0 is empty
    assert call(offsets_host=_offsets(0, 3, 3)) == EINVAL        # object 1 is empty
    assert call(query=p + 4) == EINVAL and call(bank=p + 8) == EINVAL      # 16-byte loads
    del keep


def test_normalize_and_mask_entries_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    keep, p = _host_ptr()
    off = _offsets(0, 2, 4)
    assert L.pp_descriptor_normalize(None, 2, 8, 1e-12, p, None) == EINVAL
    assert L.pp_descriptor_normalize(p, 2, 8, 1e-12, None, None) == EINVAL
    assert L.pp_descriptor_normalize(p, 0, 8, 1e-12, p, None) == EINVAL
    assert L.pp_descriptor_normalize(p, 2, 0, 1e-12, p, None) == EINVAL
    assert L.pp_descriptor_normalize(p, 2, 8, 0.0, p, None) == EINVAL
    good = dict(run_ends=p, n_runs=4, run_offset=p, run_offset_host=off, n=2, hw=35, words=2, bits=p, area=p)
    order = ("run_ends", "n_runs", "run_offset", "run_offset_host", "n", "hw", "words", "bits", "area")
    call = lambda **kw: L.pp_rle_pack_bits(*[{**good, **kw}[k] for k in order], None)  # noqa: E731
    for name in ("run_ends", "run_offset", "run_offset_host", "bits", "area"):
        assert call(**{name: None}) == EINVAL, name
    assert call(n=0) == EINVAL and call(n=4097) == EINVAL and call(n_runs=0) == EINVAL and call(hw=0) == EINVAL
    assert call(words=1) == EINVAL and call(words=3) == EINVAL   # 35 pixels are 2 words
    assert call(run_offset_host=_offsets(0, 3, 2)) == EINVAL     # decreases
    assert call(run_offset_host=_offsets(-1, 2, 4)) == EINVAL
    assert call(run_offset_host=_offsets(0, 2, 5)) == EINVAL     # past n_runs
    assert L.pp_mask_intersections(None, 2, 2, p, None) == EINVAL
    assert L.pp_mask_intersections(p, 2, 2, None, None) == EINVAL
    assert L.pp_mask_intersections(p, 0, 2, p, None) == EINVAL
    assert L.pp_mask_intersections(p, 4097, 2, p, None) == EINVAL
    assert L.pp_mask_intersections(p, 2, 0, p, None) == EINVAL
    del keep


NMS_TABLES = {
    # two overlapping pairs and a loner; 1 and 2 tie in score: the lower index is visited first
    "tie": dict(scores=[0.9, 0.8, 0.8, 0.7, 0.6], labels=[0, 0, 0, 1, 1], area=[10, 10, 10, 8, 8],
                pairs={(1, 2): 8, (0, 1): 1, (3, 4): 6}, iou=0.25),
    # IoU of (0, 1) is 2 / (5 + 5 - 2) = 0.25 exactly: kept; (0, 2) is 3 / 7: dropped
    "threshold": dict(scores=[0.9, 0.8, 0.7], labels=[0, 0, 0], area=[5, 5, 5], pairs={(0, 1): 2, (0, 2): 3}, iou=0.25),
    # a heavy overlap between different labels counts only with per_object off
    "labels": dict(scores=[0.5, 0.9, 0.7, 0.6], labels=[1, 0, 1, 0], area=[20, 20, 20, 20], pairs={(1, 2): 18, (0, 2): 15, (1, 3): 2}, iou=0.5),
    "empty_masks": dict(scores=[0.9, 0.8], labels=[0, 0], area=[0, 0], pairs={}, iou=0.25),
}
NMS_EXPECT = {("tie", True): [0, 1, 3], ("tie", False): [0, 1, 3], ("threshold", True): [0, 1], ("threshold", False): [0, 1],
              ("labels", True): [1, 2, 3], ("labels", False): [1, 3, 0], ("empty_masks", True): [0, 1], ("empty_masks", False): [0, 1]}


@pytest.mark.parametrize("per_object", [True, False])
@pytest.mark.parametrize("name", sorted(NMS_TABLES))
def test_nms_masks_equals_the_brute_force_oracle(name, per_object):
    from picopose_amd.proposals import nms_masks

    t = NMS_TABLES[name]
    n = len(t["scores"])
    inter = np.diag(t["area"]).astype(np.int32)
    for (i, j), v in t["pairs"].items():
        inter[i, j] = inter[j, i] = v
    got = nms_masks(np.float32(t["scores"]), np.int32(t["labels"]), inter, np.int32(t["area"]), t["iou"], per_object=per_object)
    assert got == po.nms(t["scores"], t["labels"], inter, t["area"], t["iou"], per_object) == NMS_EXPECT[name, per_object]
    assert len(got) <= n


def test_nms_masks_equals_the_oracle_on_random_tables():
    from picopose_amd.proposals import nms_masks

    rng = np.random.default_rng(3)
    for _ in range(30):
        n = int(rng.integers(1, 14))
        masks = rng.random((n, 40)) < 0.4
        inter = (masks.astype(np.int64) @ masks.T.astype(np.int64)).astype(np.int32)
        scores = np.round(rng.random(n), 1)                      # plenty of ties
        labels = rng.integers(0, 3, n)
        for per_object in (True, False):
            assert nms_masks(scores, labels, inter, np.diag(inter), 0.25, per_object) == po.nms(scores, labels, inter, np.diag(inter), 0.25,
                                                                                               per_object)


@pytest.mark.parametrize("C", po.C_SET)
@pytest.mark.parametrize("T", po.T_SET)
@pytest.mark.parametrize("P", po.P_SET)
def test_oracle_recovers_the_planted_labels_and_the_seed_stays_inside_the_cap(P, T, C):
    off = po.offsets_of(T)
    for topk in po.K_SET:
        q, bank, obj, view = po.planted_set(P, T, C)
        m = po.match(q, bank, off, topk)
        assert np.array_equal(m["label"], obj)
        assert undecided_labels(m, C) == 0                       # no planted case may be left out
        assert m["score"].max() <= 1 + 1e-12 and np.allclose(m["best"], m["score"].max(1))
        q, bank = po.random_set(P, T, C)
        lab, cells = po.undecided(po.match(q, bank, off, topk), C)
        assert lab <= po.UNDECIDED_CAP * P and cells <= po.UNDECIDED_CAP * P * len(T), (lab, cells)


def undecided_labels(m, C):
    return po.undecided(m, C)[0]


def test_error_bound_is_the_stated_formula():
    u = 2.0 ** -24
    for C in po.C_SET:
        g = C * u / (1 - C * u)
        assert po.err_bound(C) == pytest.approx(1.01 * (2 * g + 8 * u + 8 * u / (1 - 8 * u)), rel=1e-12)
    assert (1024 + 8) * 2.0 ** -23 < po.err_bound(1024) < (1024 + 24) * 2.0 ** -23


def test_oracle_masks_round_trip():
    for H, W in ((5, 7), (48, 64)):
        masks = po.mask_set(H, W, 17)
        segs = [po.rle_of(m) for m in masks]
        bits, area = po.pack_bits(segs)
        assert bits.shape == (17, (H * W + 31) // 32) and area.tolist() == [int(m.sum()) for m in masks]
        flat = masks[6].ravel(order="F")
        assert all(((bits[6, i // 32] >> np.uint32(i % 32)) & 1) == flat[i] for i in range(H * W))
        inter = po.intersections(segs)
        assert np.array_equal(inter, inter.T) and np.array_equal(np.diag(inter), area)
        assert area[0] == 0 and area[1] == H * W and area[2] == 1 and segs[3]["counts"][0] == 0


def test_hand_made_records_pass_the_detection_readers():
    """A record in label_proposals' format is a CNOS record with one more key: the readers of assemble_test_image take it."""
    from picopose_amd.provider.test_batch import detection_window, rle_counts, select_detections

    H, W = 64, 96
    mask = np.zeros((H, W), np.uint8)
    mask[10:30, 20:50] = 1
    records = [{"scene_id": 1, "image_id": 7, "category_id": 5, "bbox": po.mask_box(mask), "score": s, "time": 0.0,
                "segmentation": po.rle_of(mask), "view": 3} for s in (0.9, 0.6)]
    kept, seg_time = select_detections(records, 0.0)
    assert kept == [0, 1] and seg_time == 0.0
    counts = rle_counts(records[0]["segmentation"], 0)
    assert counts.sum() == H * W and counts[1::2].sum() == mask.sum()
    bbox, win = detection_window(counts, (H, W), records[0]["bbox"])
    assert bbox == win and records[0]["bbox"] == [20, 10, 30, 20]
