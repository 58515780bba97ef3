"""CPU statement of picopose_amd.provider.test_batch.assemble_test_image (TEST INFRASTRUCTURE, not collected): decode every
RLE to a dense mask with numpy, oracle.preprocess.crop_instance per kept detection, collate as
provider/bop_test_dataset.py:112-144 does (torch.FloatTensor / IntTensor of each entry, stacked, then the DataLoader's
leading dimension of 1).  Also the RLE encoder the tests use.

COCO's RLE is restated from its published definition (pycocotools' maskApi.c: rleEncode, rleToString, rleFrString);
pycocotools itself is not available, so parity with it is unpinned."""
import numpy as np

from oracle import preprocess as op


def mask_to_counts(mask):
    """(h, w) binary mask -> COCO run lengths (column-major, first run counts zeros and may be 0)."""
    flat = np.asarray(mask).astype(bool).ravel(order="F")
    counts, cur, run = [], False, 0
    for v in flat:
        if v != cur:
            counts.append(run)
            cur, run = v, 0
        run += 1
    counts.append(run)
    return counts


def mask_to_counts_fast(mask):
    """The same by numpy (for frame-sized masks); checked against mask_to_counts in the CPU tests."""
    flat = np.asarray(mask).astype(np.int8).ravel(order="F")
    edges = np.nonzero(np.diff(flat))[0] + 1
    bounds = np.concatenate(([0], edges, [flat.size]))
    counts = np.diff(bounds).tolist()
    return ([0] + counts) if flat[0] else counts


def counts_to_string(counts):
    """rleToString: differences from the fourth count on, five bits per character, bit 0x20 = more, sign in bit 0x10."""
    out = []
    for i, c in enumerate(counts):
        x = int(c) - (int(counts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            out.append(chr(ch + 48))
    return "".join(out)


def string_to_counts(s):
    """rleFrString, character by character."""
    if isinstance(s, (bytes, bytearray)):
        s = s.decode("ascii")
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def decode(segmentation):
    """{"size": [h, w], "counts": list | str | bytes} -> dense (h, w) uint8 mask."""
    h, w = segmentation["size"]
    counts = segmentation["counts"]
    if isinstance(counts, (str, bytes, bytearray)):
        counts = string_to_counts(counts)
    counts = np.asarray(counts, np.int64)
    assert counts.sum() == h * w and (counts >= 0).all()
    flat = np.repeat(np.arange(len(counts)) & 1, counts).astype(np.uint8)
    return flat.reshape((h, w), order="F")


def collate(image_u8, detections, K, obj_idxs, scene_id, img_id, seg_filter_score=0.0, img_size=224, pts_size=64,
            minimum_n_point=8, rgb_mask_flag=False):
    """-> dict of numpy arrays with the shapes and dtypes of the collated reference batch, or None if nothing is kept."""
    img = np.asarray(image_u8)
    if img.ndim == 2:
        img = np.concatenate([img[:, :, None]] * 3, axis=2)
    img = img[..., :3]
    rows = []
    for det in detections:
        if det["score"] > seg_filter_score:
            r = op.crop_instance(img, decode(det["segmentation"]), det["bbox"], img_size, pts_size, minimum_n_point, rgb_mask_flag)
            rows.append({"score": np.array([det["score"]], np.float32), "obj_id": np.array([det["category_id"]], np.int32),
                         "obj_idx": np.array([obj_idxs[det["category_id"]]], np.int32), "real_pts2d": r["pts2d"].astype(np.float32),
                         "real_rgb": r["rgb"].astype(np.float32), "real_bbox": np.asarray(r["bbox"], np.float32),
                         "real_mask": r["mask"].astype(np.float32), "real_M": r["M"].astype(np.float32),
                         "real_K": np.array(K, np.float64).reshape(3, 3).astype(np.float32), "real_pose": np.eye(4, dtype=np.float32)})
    if not rows:
        return None
    out = {k: np.stack([r[k] for r in rows])[None] for k in rows[0]}
    out["scene_id"] = np.array([[scene_id]], np.int32)
    out["img_id"] = np.array([[img_id]], np.int32)
    out["seg_time"] = np.array([[detections[0]["time"]]], np.float32)
    return out


# ---- seeded scenes shared by the CPU and GPU tests ---------------------------------------------------------------------------

def blob(rng, H, W, holes=0.1):
    """An elliptic blob with `holes` of its pixels knocked out."""
    h, w = int(rng.integers(max(4, H // 8), max(6, H // 2))), int(rng.integers(max(4, W // 8), max(6, W // 2)))
    y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((H, W), np.uint8)
    m[y:y + h, x:x + w] = (((yy - (h - 1) / 2) / (h / 2)) ** 2 + ((xx - (w - 1) / 2) / (w / 2)) ** 2 <= 1) & (rng.random((h, w)) >= holes)
    return m


def record(mask, score, obj_id, time=0.25, compressed=True, bbox=None):
    counts = mask_to_counts_fast(mask)
    if bbox is None:
        ys, xs = np.nonzero(mask)
        bbox = [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)] if len(ys) else [0, 0, 4, 4]
    return {"scene_id": 1, "image_id": 7, "category_id": int(obj_id), "bbox": bbox, "score": float(score), "time": float(time),
            "segmentation": {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": counts_to_string(counts) if compressed else counts}}


def scene(seed, H, W, n, compressed=True):
    """A frame and n + 1 detection records, n of them above the score filter: blobs with holes, smooth blobs, one on the
    small-mask branch (3 pixels: the window comes from its detection box), one whose window is clamped at a frame border
    and one at or below the filter score (dropped).  With n = 1 the kept one alternates between the small-mask and the
    clamped kind by seed.  -> (image, detections, K, obj_idxs)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.clip(128 + 70 * np.sin(yy / 7.0)[..., None] * np.cos(xx / 11.0)[..., None] + rng.normal(0, 30, (H, W, 3)), 0, 255).astype(np.uint8)
    dets = []

    def small():
        m = np.zeros((H, W), np.uint8)
        y, x = int(rng.integers(0, H - 1)), int(rng.integers(0, W - 2))
        m[y, x:x + 2] = 1
        m[y + 1, x] = 1
        bw, bh = int(rng.integers(3, max(4, W // 3))), int(rng.integers(3, max(4, H // 3)))
        return m, [max(0, x - bw // 2), max(0, y - bh // 2), bw, bh]

    def clamped(k):
        m = np.zeros((H, W), np.uint8)
        s, t = max(3, min(H, W) // 3), max(2, min(H, W) // 8)
        if k % 4 == 0:
            m[0:t, W // 4:W // 4 + s] = 1           # wide and at the top: the square window is pushed down
        elif k % 4 == 1:
            m[H - t:H, W // 3:W // 3 + s] = 1       # bottom
        elif k % 4 == 2:
            m[H // 4:H // 4 + s, 0:t] = 1           # left
        else:
            m[H // 3:H // 3 + s, W - t:W] = 1       # right
        return m, None

    for j in range(n):
        if n == 1:
            kind = seed % 2
        else:
            kind = j if j < 2 else 2 + j % 2                 # 0 small mask, 1 clamped, 2 blob with holes, 3 smooth blob
        if kind == 0:
            m, bbox = small()
        elif kind == 1:
            m, bbox = clamped(seed + j)
        else:
            m, bbox = blob(rng, H, W, holes=0.1 if kind == 2 else 0.0), None
        dets.append(record(m, 0.9 - 0.02 * j, 1 + j % 3, compressed=compressed, bbox=bbox))
        if j == 0:
            dets.append(record(blob(rng, H, W), 0.0, 2, compressed=compressed))     # at the filter score: dropped
    K = [572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0]
    return img, dets, K, {1: 2, 2: 0, 3: 1}
