"""Detection batch of one test image on the device — the reference's provider/bop_test_dataset.py:112-207
(`BOPTestset.__getitem__` + `get_instance`) from one decoded image and its CNOS detection records to the `data` dict that
`pipeline.infer_image` walks.

File reading (JSON, PNG/JPEG) stays with the caller.  The masks stay run lengths from the record to the kernel: the host
reads pixel count and extent off the runs, the device tests membership by a search over the cumulative run ends
(csrc/pp_detect.hip, `pp_detections_crop`); no frame-sized mask is built on either side.  The encoding, its decoder and the
run tables are masks.py's, and so is the `pp_detections_crop` launch (`RunTable.crop`).  The frame goes up once, the
small arrays (runs, windows, ids, scores, `M`, `pts2d`, boxes, `K`, poses) in one pinned buffer and one copy; one launch
crops, resizes and normalises every kept detection into the collated tensors.  Nothing in the call waits for the device.

Stated differences from the reference:
- an image whose detections are all at or below `seg_filter_score` gives `None` (the reference raises IndexError at
  `instances[0]`, bop_test_dataset.py:139);
- the two `cv2.resize` legs follow OpenCV's published definitions, as for `utils.preprocess.crop_instance`, whose outputs
  this call reproduces bit for bit."""
import contextlib

import numpy as np
import torch

from ..masks import RunTable, check_frame, check_window, rle_area_extent, rle_counts, run_ends, run_words
from ..utils.preprocess import _square, get_square_bbox


def detection_window(counts, size, det_bbox_xywh, minimum_n_point=8):
    """bop_test_dataset.py:169-173 on run lengths -> (bbox, window): with more than `minimum_n_point` mask pixels both are
    get_bbox(mask); otherwise the window is get_square_bbox of the detection box while `bbox` — which feeds M_crop and is
    returned — stays the detection's [x, y, w, h] (the upstream quirk `utils.preprocess.crop_instance` keeps too)."""
    h, w = size
    area, extent = rle_area_extent(counts, h)
    if area > minimum_n_point:
        rmin, rmax, cmin, cmax = extent
        bbox = _square(rmin, rmax + 1, cmin, cmax + 1, h, w)
        return bbox, bbox
    b = list(det_bbox_xywh)
    return b, get_square_bbox([b[1], b[1] + b[3], b[0], b[0] + b[2]], (h, w))


def select_detections(detections, seg_filter_score=0.0):
    """bop_test_dataset.py:116-117, 143: -> (indices of the detections with score > seg_filter_score, in the given order;
    seg_time = the FIRST record's `time`, whether that record is kept or not)."""
    if len(detections) == 0:
        raise ValueError("no detections")
    return [i for i, d in enumerate(detections) if d["score"] > seg_filter_score], float(detections[0]["time"])


def crop_affines(bboxes, windows, img_size=224, pts_size=64):
    """`real_M` (n, 3, 3) float32 and `real_pts2d` (n, P, P, 2) float64 of bop_test_dataset.py:181-196 for n detections at
    once, with crop_instance's own expressions: float32 M_resize @ M_crop, np.linalg.inv of the float32 M, float64 product
    with the lookup grid of utils/torch_utils.py:287-295 (y first)."""
    n = len(bboxes)
    win = np.asarray(windows, np.int64).reshape(n, 4)
    M_crop = np.zeros((n, 3, 3), np.float32)
    M_resize = np.zeros((n, 3, 3), np.float32)
    M_crop[:, 0, 0] = M_crop[:, 1, 1] = M_crop[:, 2, 2] = M_resize[:, 2, 2] = 1
    M_crop[:, 0, 2] = [-b[2] for b in bboxes]
    M_crop[:, 1, 2] = [-b[0] for b in bboxes]
    M_resize[:, 0, 0] = img_size / (win[:, 1] - win[:, 0])
    M_resize[:, 1, 1] = img_size / (win[:, 3] - win[:, 2])
    M = M_resize @ M_crop
    patch = img_size / pts_size
    x = np.arange(0, img_size, patch, dtype=np.float32) + patch / 2
    yy, xx = np.meshgrid(x, x, indexing="ij")
    pts = np.concatenate((np.stack([yy, xx], axis=2), np.ones((pts_size, pts_size, 1))), axis=2)
    p = np.linalg.inv(M) @ pts.reshape(-1, 3).transpose(1, 0)
    pts2d = (p[:, :2] / p[:, 2:]).transpose(0, 2, 1).reshape(n, pts_size, pts_size, 2)
    return M, pts2d


def _frame_u8(image_u8):
    img = np.asarray(image_u8)
    if img.ndim == 2:                                      # utils/data_utils.py:243-244: a grey image becomes three equal channels
        img = np.stack([img, img, img], axis=2)
    if img.ndim != 3 or img.shape[2] < 3 or img.dtype != np.uint8:
        raise ValueError(f"image must be (H, W), (H, W, 3) or (H, W, 4) uint8, got {img.shape} {img.dtype}")
    return img[..., :3]


def assemble_test_image(image_u8, detections, K, obj_idxs, *, scene_id, img_id, seg_filter_score=0.0, img_size=224, pts_size=64,
                        minimum_n_point=8, rgb_mask_flag=False, device="cuda", stream=None):
    """One decoded test image + its CNOS detection records -> the `data` dict of `pipeline.infer_image`, i.e. what
    `BOPTestset.__getitem__` returns after the DataLoader's collation with batch size 1 (bop_test_dataset.py:112-144):
      score (1,n,1) f32, obj_id / obj_idx (1,n,1) int32, real_pts2d (1,n,P,P,2), real_rgb (1,n,3,S,S), real_bbox (1,n,4),
      real_mask (1,n,S,S), real_M (1,n,3,3), real_K (1,n,3,3), real_pose (1,n,4,4) = identity, all f32; scene_id, img_id
      (1,1) int32, seg_time (1,1) f32 — tensors on `device`.
    image_u8: (H, W, 3) uint8 as loaded; (H, W) grey is repeated over three channels, a fourth channel is dropped.
    detections: the image's records, each with `score`, `category_id`, `bbox` [x, y, w, h], `time` and `segmentation`
    (`rle_counts` lists the accepted forms), already sorted and cut as the caller wants them (bop_test_dataset.py:97-107).
    Those with score > seg_filter_score are kept, in order; None if none is.  K: the image's `cam_K` (9 values);
    obj_idxs: object id -> index into the template bank (a mapping, or anything indexable by the id).
    The defaults are the reference's config/base.yaml `test_dataset` block.
    Everything is enqueued on `stream` (default: the current stream) without waiting for it: a caller can assemble image
    i + 1 while image i runs and pass it to `infer_image(..., next_data=...)`.  A caller that consumes the tensors on another
    stream orders the two streams itself.  ValueError names the detection (its index in `detections`) whose RLE is
    malformed, whose mask size is not the image's, or whose crop window is empty."""
    frame = _frame_u8(image_u8)
    H, W = frame.shape[:2]
    check_frame(H, W)
    kept, seg_time = select_detections(detections, seg_filter_score)
    if not kept:
        return None
    n, S, P = len(kept), int(img_size), int(pts_size)
    K = np.array(K, dtype=np.float64).reshape(3, 3)
    runs, bboxes, windows = [], [], []
    for i in kept:
        det = detections[i]
        counts = rle_counts(det["segmentation"], i, "detection", (H, W))
        bbox, win = detection_window(counts, (H, W), det["bbox"], minimum_n_point)
        check_window(win, H, W, i, "detection")
        runs.append(run_ends(counts))
        bboxes.append(bbox)
        windows.append(win)
    M, pts2d = crop_affines(bboxes, windows, S, P)
    run_words_h, run_offset = run_words(runs)
    window = np.asarray(windows, np.int32)
    n_tab = len(run_words_h)

    # ---- one staging buffer of 4-byte words: the run tables and the other int32 arrays, then the float32 tensors as
    # torch.FloatTensor(...) rounds them
    ints = [run_words_h, window.ravel(),
            [int(detections[i]["category_id"]) for i in kept], [int(obj_idxs[detections[i]["category_id"]]) for i in kept],
            [int(scene_id)], [int(img_id)]]
    floats = [np.asarray([detections[i]["score"] for i in kept], np.float32), pts2d.astype(np.float32).ravel(),
              np.asarray(bboxes, np.float32).ravel(), M.ravel(), np.tile(K.astype(np.float32).ravel(), n),
              np.tile(np.eye(4, dtype=np.float32).ravel(), n), np.asarray([seg_time], np.float32)]
    n_int = sum(len(a) for a in ints)
    words_h = torch.empty(n_int + sum(len(a) for a in floats), dtype=torch.int32, pin_memory=True)
    wv = words_h.numpy()
    wv[:n_int] = np.concatenate(ints)
    wv[n_int:].view(np.float32)[:] = np.concatenate(floats)
    frame_h = torch.empty((H, W, 3), dtype=torch.uint8, pin_memory=True)
    frame_h.numpy()[:] = frame

    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        frame_d = frame_h.to(device, non_blocking=True)
        words = words_h.to(device, non_blocking=True)
        rgb = torch.empty((1, n, 3, S, S), dtype=torch.float32, device=device)
        mask = torch.empty((1, n, S, S), dtype=torch.float32, device=device)
        RunTable.from_words(words, run_offset).crop(frame_d, words[n_tab:n_tab + 4 * n], window, S, rgb_mask_flag, rgb, mask)
    data = {"real_rgb": rgb, "real_mask": mask}
    o = n_tab + 4 * n
    for k, shape in (("obj_id", (1, n, 1)), ("obj_idx", (1, n, 1)), ("scene_id", (1, 1)), ("img_id", (1, 1))):
        m = int(np.prod(shape))
        data[k] = words[o:o + m].view(shape)
        o += m
    fl = words.view(torch.float32)
    for k, shape in (("score", (1, n, 1)), ("real_pts2d", (1, n, P, P, 2)), ("real_bbox", (1, n, 4)), ("real_M", (1, n, 3, 3)),
                     ("real_K", (1, n, 3, 3)), ("real_pose", (1, n, 4, 4)), ("seg_time", (1, 1))):
        m = int(np.prod(shape))
        data[k] = fl[o:o + m].view(shape)
        o += m
    return data
