"""CPU oracle of the training-pair assembly (picopose_amd/provider/training_batch.py, csrc/pp_augment.hip) — test helper,
numpy only.

Restates, from their definitions, every augmenter of the gdrnpp recipe on a uint8 HWC crop, whole programs, the 8-bit
cv::resize (INTER_LINEAR fixed point, INTER_AREA for an exact 2x downscale, INTER_NEAREST), the CLIP normalisation, and
the reference's `process_real` / `process_template` (provider/training_dataset.py:173-316) with the draws supplied by the
caller.  Rows 3-6 are checked against PIL.ImageEnhance itself (tests/test_train_batch_cpu.py); the other rows follow
imgaug 0.4.0 / OpenCV as recalled (neither is installed), with the counter-hash noise and dropout of include/picopose_hip.h."""
import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
F = np.float32


# ---- counter-based hash (uint32 arithmetic wraps) ----------------------------------------------------------------
def mix(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def hash3(seed, a, b):
    a = np.asarray(a, np.uint32)
    b = np.broadcast_to(np.asarray(b, np.uint32), a.shape)
    return mix(np.uint32(seed) ^ mix(a ^ mix(b + np.uint32(0x9e3779b9))))


# ---- the augmenters -----------------------------------------------------------------------------------------------
def pil_l(img):
    i = img.astype(np.int64)
    return (i[..., 0] * 19595 + i[..., 1] * 38470 + i[..., 2] * 7471 + 0x8000) >> 16


def blend(d, v, f):
    """PIL Image.blend(degenerate, image, f) on uint8: clip(trunc(d + f (v - d))), float32, one rounding per operation."""
    d = np.asarray(d).astype(F)
    t = d + F(f) * (np.asarray(v).astype(np.int64) - np.asarray(d).astype(np.int64)).astype(F)
    return np.clip(np.trunc(t), 0, 255).astype(np.uint8)


def smooth(img):
    """PIL ImageFilter.SMOOTH on uint8: round(sum / 13) of [[1,1,1],[1,5,1],[1,1,1]] on the interior, border copied."""
    i = img.astype(np.int64)
    H, W = i.shape[:2]
    out = i.copy()
    if H >= 3 and W >= 3:
        s = sum(i[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) + 4 * i[1:-1, 1:-1]
        out[1:-1, 1:-1] = (s + 6) // 13
    return out


def sharpness(img, f):
    return blend(smooth(img), img, f)


def contrast(img, f):
    return blend(np.full_like(img, int(pil_l(img).mean() + 0.5)), img, f)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def color(img, f):
    return blend(np.repeat(pil_l(img)[..., None], 3, 2), img, f)


def dropout(img, seed):
    h, w = img.shape[:2]
    gh, gw = max(h * 5 // 100, 3), max(w * 5 // 100, 3)
    cy = np.arange(h) * gh // h
    cx = np.arange(w) * gw // w
    cell = cy[:, None] * gw + cx[None, :]
    drop = hash3(seed, cell, 0xD0) < np.uint32(858993459)
    out = img.copy()
    out[drop] = 0
    return out


def taps(sigma):
    if sigma <= 1e-3:
        return np.array([1.0]), np.array([256])
    k = max(5, int(3.3 * sigma))
    if k % 2 == 0:
        k += 1
    x = np.arange(-(k // 2), k // 2 + 1, dtype=np.float64)
    g = np.exp(-x * x / (2 * sigma * sigma))
    g = g / g.sum()
    q = np.rint(g * 256).astype(np.int64)
    q[k // 2] = 0
    q[k // 2] = 256 - q.sum()
    return g, q


def reflect101(p, n):
    if n == 1:
        return np.zeros_like(p)
    p = np.array(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def gaussian_blur(img, sigma):
    """8-bit fixed point: quantised taps q (each axis sums to 256), BORDER_REFLECT_101, exact integer 2-D sum, one rounding."""
    _, q = taps(sigma)
    r = len(q) // 2
    if r == 0:
        return img.copy()
    h, w = img.shape[:2]
    i = img.astype(np.int64)
    ys, xs = np.arange(h), np.arange(w)
    rows = sum(q[j + r] * i[:, reflect101(xs + j, w)] for j in range(-r, r + 1))
    acc = sum(q[k + r] * rows[reflect101(ys + k, h)] for k in range(-r, r + 1))
    return ((acc + 32768) >> 16).astype(np.uint8)


def add(img, a):
    return np.clip(img.astype(np.int64) + np.asarray(a, np.int64), 0, 255).astype(np.uint8)


def invert(img, flags):
    return np.where(np.asarray(flags, bool), 255 - img, img).astype(np.uint8)


def multiply(img, m):
    return np.clip(np.rint(img.astype(F) * np.asarray(m, F)), 0, 255).astype(np.uint8)


def noise(img, seed):
    h, w = img.shape[:2]
    a = (np.arange(h * w, dtype=np.int64)[:, None] * 3 + np.arange(3)).reshape(h, w, 3)
    s = np.zeros((h, w, 3), np.int64)
    for k in range(3):
        hh = hash3(seed, a.astype(np.uint32), k).astype(np.int64)
        s += (hh & 255) + ((hh >> 8) & 255) + ((hh >> 16) & 255) + (hh >> 24)
    n = ((2 * s - 12 * 255) * 10 + 256) >> 9
    return np.clip(img.astype(np.int64) + n, 0, 255).astype(np.uint8)


def linear_contrast(img, alpha):
    return np.clip(np.trunc(F(127) + np.asarray(alpha, F) * (img.astype(F) - F(127))), 0, 255).astype(np.uint8)


def grayscale(img, alpha):
    i = img.astype(np.int64)
    g = ((i[..., 0] * 4899 + i[..., 1] * 9617 + i[..., 2] * 1868 + 8192) >> 14).astype(F)[..., None]
    a = F(alpha)
    return np.clip(np.rint(a * g + (F(1) - a) * img.astype(F)), 0, 255).astype(np.uint8)


def apply_op(img, row, params, seed):
    if row == 1:
        return dropout(img, seed)
    if row == 2:
        return gaussian_blur(img, params[0])
    if row in (3, 4, 5, 6):
        return (sharpness, contrast, brightness, color)[row - 3](img, params[0])
    if row == 7:
        return add(img, params)
    if row == 8:
        return invert(img, params)
    if row in (9, 10):
        return multiply(img, params)
    if row == 11:
        return noise(img, seed)
    if row == 12:
        return linear_contrast(img, params)
    if row == 13:
        return grayscale(img, params[0])
    raise ValueError(row)


def run_program(img, program):
    for row, params in program.ops:
        img = apply_op(img, row, params, program.seed)
    return img


# ---- resize and normalise (cv::resize on CV_8U) --------------------------------------------------------------------
def _linear_coeffs(S, n, clamp_edges):
    d = np.arange(S, dtype=np.float64)
    f = ((d + 0.5) * (1.0 / (S / n)) - 0.5).astype(F)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F)).astype(F)
    if clamp_edges:
        f = np.where((s < 0) | (s >= n - 1), F(0), f)
        s = np.clip(s, 0, n - 1)
    c0 = np.clip(np.rint((F(1) - f) * F(2048)), -32768, 32767).astype(np.int64)
    c1 = np.clip(np.rint(f * F(2048)), -32768, 32767).astype(np.int64)
    return s, c0, c1


def resize_linear_u8(img, S):
    """INTER_LINEAR, OpenCV's scalar fixed-point path (INTER_AREA for an exact 2x downscale)."""
    h, w = img.shape[:2]
    i = img.astype(np.int64)
    if h == 2 * S and w == 2 * S:
        return ((i[0::2, 0::2] + i[0::2, 1::2] + i[1::2, 0::2] + i[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, a0, a1 = _linear_coeffs(S, w, True)
    sx1 = np.minimum(sx + 1, w - 1)
    sy, b0, b1 = _linear_coeffs(S, h, False)
    r0, r1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    hor = i[:, sx] * a0[None, :, None] + i[:, sx1] * a1[None, :, None]
    v = b0[:, None, None] * hor[r0] + b1[:, None, None] * hor[r1]
    return np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def resize_nearest(m, S):
    h, w = m.shape[:2]
    ys = np.minimum(np.floor(np.arange(S) * (1.0 / (S / h))).astype(np.int64), h - 1)
    xs = np.minimum(np.floor(np.arange(S) * (1.0 / (S / w))).astype(np.int64), w - 1)
    return m[ys][:, xs]


def to_tensor_normalize(rgb_u8):
    """transforms.ToTensor(rgb / 255) + Normalize(CLIP) in float64, then .float()."""
    x = (rgb_u8 / 255).transpose(2, 0, 1)
    return ((x - np.asarray(CLIP_MEAN)[:, None, None]) / np.asarray(CLIP_STD)[:, None, None]).astype(np.float32)


# ---- the reference's boxes, crops and views ----------------------------------------------------------------------
def get_bbox(label, size_ratio=1.0):
    """utils/data_utils.py:131-165."""
    rows, cols = np.any(label, axis=1), np.any(label, axis=0)
    rmin, rmax = np.where(rows)[0][[0, -1]]
    cmin, cmax = np.where(cols)[0][[0, -1]]
    rmax += 1
    cmax += 1
    img_width, img_length = label.shape
    r_b = min(max(rmax - rmin, cmax - cmin), min(img_width, img_length)) * size_ratio
    c_b = r_b
    center = [int((rmin + rmax) / 2), int((cmin + cmax) / 2)]
    rmin, rmax = center[0] - int(r_b / 2), center[0] + int(r_b / 2)
    cmin, cmax = center[1] - int(c_b / 2), center[1] + int(c_b / 2)
    if rmin < 0:
        rmax, rmin = rmax - rmin, 0
    if cmin < 0:
        cmax, cmin = cmax - cmin, 0
    if rmax > img_width:
        rmin, rmax = rmin - (rmax - img_width), img_width
    if cmax > img_length:
        cmin, cmax = cmin - (cmax - img_length), img_length
    return [int(rmin), int(rmax), int(cmin), int(cmax)]


def m_of(bbox, img_size):
    y1, y2, x1, x2 = bbox
    M_crop = np.array([[1, 0, -bbox[2]], [0, 1, -bbox[0]], [0, 0, 1]], dtype=np.float32)
    M_resize = np.array([[img_size / (y2 - y1), 0, 0], [0, img_size / (x2 - x1), 0], [0, 0, 1]], dtype=np.float32)
    return M_resize @ M_crop


def process_real(s, program, img_size=224, rgb_mask_flag=False, size_ratio=1.0):
    """training_dataset.py:200-248 on a decoded sample, the augmentation given as a program (None: not applied)."""
    mask = np.asarray(s["mask"])
    bbox = get_bbox(mask > 0, size_ratio)
    y1, y2, x1, x2 = bbox
    mask = mask[y1:y2, x1:x2]
    image = np.asarray(s["rgb"]).astype(np.uint8)
    rgb = image[..., ::-1][y1:y2, x1:x2, :]
    if program is not None:
        rgb = run_program(np.ascontiguousarray(rgb), program)
    if rgb_mask_flag:
        rgb = rgb * (mask[:, :, None] > 0).astype(np.uint8)
    rgb = resize_linear_u8(rgb, img_size)
    mask = resize_nearest(mask.astype(int), img_size)
    depth = np.asarray(s["depth"]).astype(np.float32)
    depth = depth * s["depth_scale"] / 1000.0
    pose = np.eye(4)
    pose[:3, :3] = np.array(s["cam_R_m2c"]).reshape(3, 3).astype(np.float32)
    pose[:3, 3] = np.array(s["cam_t_m2c"]).reshape(3).astype(np.float32) / 1000.0
    return {"full_depth": depth, "rgb": to_tensor_normalize(rgb), "mask": mask, "bbox": bbox, "M": m_of(bbox, img_size),
            "K": np.array(s["K"]).reshape(3, 3), "pose": pose}


def process_template(s, program, img_size=224, rgb_mask_flag=False, size_ratio=1.0, templates_K=None):
    """training_dataset.py:269-316 on a decoded sample."""
    rgba = np.asarray(s["tem_rgba"])
    rgb = rgba[..., :3]
    mask = (rgba[..., 3] / 255).astype(np.float32)
    bbox = get_bbox(mask > 0, size_ratio)
    y1, y2, x1, x2 = bbox
    mask = mask[y1:y2, x1:x2]
    rgb = rgb.astype(np.uint8)[..., ::-1][y1:y2, x1:x2, :]
    if program is not None:
        rgb = run_program(np.ascontiguousarray(rgb), program)
    if rgb_mask_flag:
        rgb = rgb * (mask[:, :, None] > 0).astype(np.uint8)
    rgb = resize_linear_u8(rgb, img_size)
    mask = resize_nearest(mask.astype(int), img_size)
    depth = np.asarray(s["tem_depth"]) * 0.1 / 1000.0
    object_pose = np.array(s["tem_pose"])
    object_pose[:3, 3] = object_pose[:3, 3] * 0.1 / 1000.0
    K = templates_K if templates_K is not None else np.array([572.4114, 0.0, 320, 0.0, 573.57043, 240, 0.0, 0.0, 1.0]).reshape((3, 3))
    return {"full_depth": depth, "rgb": to_tensor_normalize(rgb), "mask": mask, "bbox": bbox, "M": m_of(bbox, img_size), "K": K,
            "pose": object_pose}


def collate(samples, real_programs, tem_programs, **kw):
    """read_data (training_dataset.py:152-169) + the DataLoader's stacking -> numpy float32 arrays per key."""
    out = {}
    for pre, fn, progs in (("real_", process_real, real_programs), ("tem_", process_template, tem_programs)):
        views = [fn(s, p if p is not None and p.applied else None, **kw) for s, p in zip(samples, progs)]
        for k in ("full_depth", "rgb", "bbox", "mask", "M", "K", "pose"):
            out[pre + k] = np.stack([np.asarray(v[k], np.float32) for v in views])
    return out


def sample_template_views(object_rot, template_poses, topk=5):
    """training_dataset.py:320-330 without the final draw (R_opencv2R_opengl of utils/template_utils.py:56-62)."""
    transform = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]])
    tem = np.matmul(np.tile(transform, (template_poses.shape[0], 1, 1)), template_poses[:, :3, :3])
    locations = tem[:, 2, :3]
    query = np.matmul(transform, object_rot)[2, :3]
    distances = np.linalg.norm(query - locations, axis=1)
    return np.argsort(distances)[:topk]
