"""Training-pair assembly on the device — the reference's provider/training_dataset.py:137-331 (`read_data`,
`process_real`, `process_template`, `sample_template` and the gdrnpp colour augmentation) from decoded arrays to the
collated `end_points` that `Net.forward` consumes in train mode.

File reading and decoding stay with the caller, as for the test-time crops (utils/preprocess.py).  The host draws the
random choices and computes boxes, `M`, K and poses in numpy; the pixels go through csrc/pp_augment.hip:
`pp_augment_execute` runs each image's augmentation *program* (the augmenters that fired, in their drawn order, with their
drawn parameters), `pp_augment_resize` does the 8-bit INTER_LINEAR resize and the CLIP normalisation, `pp_depth_u16_*`
convert the depth frames.  tests/train_batch_oracle.py restates every step in numpy, bit for bit.

Stated deviations from the reference:
- the draws are statistically those of the recipe (gates, order, parameter ranges, per-channel choices), not imgaug's
  random stream; the same numpy Generator state gives the same batch;
- AdditiveGaussianNoise is an Irwin-Hall sum of 12 hashed bytes scaled to std ~10 (not a true normal) and CoarseDropout's
  cells come from the same counter-based hash (include/picopose_hip.h);
- the augmenters of rows 1, 2 and 7-13 follow imgaug 0.4.0's definitions as restated in `ColorAugmentor`'s docstring
  (imgaug and cv2 are not available to pin them); rows 3-6 equal PIL's ImageEnhance bit for bit;
- the resize is OpenCV's scalar fixed-point INTER_LINEAR (its SIMD vertical pass may round 1 LSB differently).
"""
import ctypes
from typing import NamedTuple

import numpy as np
import torch

from .. import _lib
from ..utils.preprocess import CLIP_MEAN, CLIP_STD, get_bbox

OP_WORDS, IMG_WORDS, MAX_OPS, MAX_PASSES = 8, 20, 13, 4
ROW_NAMES = ("CoarseDropout", "GaussianBlur", "EnhanceSharpness", "EnhanceContrast", "EnhanceBrightness", "EnhanceColor", "Add",
             "Invert", "MultiplyPerChannel", "Multiply", "AdditiveGaussianNoise", "LinearContrast", "Grayscale")
GATES = (0.5, 0.4, 0.3, 0.3, 0.5, 0.3, 0.5, 0.3, 0.5, 0.5, 0.1, 0.5, 0.5)   # training_dataset.py:87-103, Sometimes(p, ...)
PASS_ROWS = (2, 3, 4)        # blur and sharpness read neighbours, contrast the whole image: each starts a pass
APPLY_P = 0.8                # training_dataset.py:216 `np.random.rand() < 0.8`
TEMPLATES_K = np.array([572.4114, 0.0, 320, 0.0, 573.57043, 240, 0.0, 0.0, 1.0]).reshape((3, 3))   # training_dataset.py:54-56
MIN_MASK_PIXELS = 32         # training_dataset.py:210


class Program(NamedTuple):
    """One image's augmentation: `applied` = the 0.8 gate, `seed` (uint32) keys the dropout cells and the noise, `ops` =
    ((row, params), ...) in execution order, row 1..13 of the recipe (ROW_NAMES)."""
    applied: bool
    seed: int
    ops: tuple


EMPTY = Program(False, 0, ())


def gaussian_taps(sigma):
    """GaussianBlur kernel of the recipe: ksize = odd(max(5, int(3.3 sigma))), no-op (radius 0) for sigma <= 1e-3; the
    normalised float kernel exp(-i^2 / 2 sigma^2) quantised to 8 bits (round), the centre tap taking the remainder so each
    axis sums to 256.  -> (radius, (q0, q1, q2, q3, q4))."""
    if sigma <= 1e-3:
        return 0, (256, 0, 0, 0, 0)
    k = max(5, int(3.3 * sigma))
    k += 1 - k % 2
    r = k // 2
    x = np.arange(0, r + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    g /= g[0] + 2.0 * g[1:].sum()
    q = np.rint(g * 256.0).astype(np.int64)
    q[0] = 256 - 2 * q[1:].sum()
    return r, tuple(int(v) for v in q) + (0,) * (4 - r)


class ColorAugmentor:
    """training_dataset.py:87-103: Sequential of 13 Sometimes(p, augmenter), random_order=True, applied with p 0.8.

    `sample(n)` draws, from the caller's numpy Generator, for each image: the 0.8 gate, the 13 gates, a uniformly random order,
    every parameter and per-channel choice, and a uint32 seed.  The draws are statistically those of the recipe, not
    imgaug's random stream.  Parameters are held as float32 (the kernels' precision).  What each row computes on a uint8
    HWC crop v (channels in the crop's order; tests/train_batch_oracle.py restates it):
      1 CoarseDropout(p=0.2, size_percent=0.05): grid max(h*5//100, 3) x max(w*5//100, 3), nearest cell y*gh//h, x*gw//w,
        a cell drops (all channels -> 0) when hash < 0.2 * 2^32
      2 GaussianBlur(sigma ~ U(0,3)): gaussian_taps, BORDER_REFLECT_101, (sum q_i q_j v + 2^15) >> 16
      3-6 pillike.Enhance{Sharpness U(0,50), Contrast U(0.2,50), Brightness U(0.1,6), Color U(0,20)}: PIL's
        clip(trunc(d + f (v - d))) in float32, d = SMOOTH filter / int(mean(L) + 0.5) / 0 / L (PIL's ImageEnhance)
      7 Add(U{-25..25}, per_channel=0.3): clip(v + a)
      8 Invert(0.2, per_channel=True): 255 - v on each chosen channel
      9, 10 Multiply(U(0.6,1.4), per_channel=0.5 / False): clip(rint(f32(v) * m))
      11 AdditiveGaussianNoise(scale=10, per_channel=True): clip(v + n), n the hashed Irwin-Hall integer of
        include/picopose_hip.h (std ~10; not a true normal)
      12 LinearContrast(U(0.5,2.2), per_channel=0.3): clip(trunc(127 + a (v - 127))) in float32
      13 Grayscale(alpha ~ U(0,1)): g = (4899 v0 + 9617 v1 + 1868 v2 + 2^13) >> 14 (cv2 RGB2GRAY, 8-bit),
        clip(rint(a g + (1 - a) v)) in float32."""

    def __init__(self, generator):
        self.generator = generator

    def sample(self, n):
        g = self.generator
        applied = g.random(n) < APPLY_P
        fired = g.random((n, 13)) < np.asarray(GATES)
        order = np.argsort(g.random((n, 13)), axis=1)
        seed = g.integers(0, 1 << 32, n, dtype=np.uint64)
        f32 = np.float32
        sigma = g.uniform(0.0, 3.0, n).astype(f32)
        enh = np.stack([g.uniform(0.0, 50.0, n), g.uniform(0.2, 50.0, n), g.uniform(0.1, 6.0, n), g.uniform(0.0, 20.0, n)], 1).astype(f32)

        def per_channel(p, values):
            pc = g.random(n) < p
            values[~pc] = values[~pc, :1]
            return values

        add = per_channel(0.3, g.integers(-25, 26, (n, 3)))
        inv = (g.random((n, 3)) < 0.2).astype(np.int64)
        mul_pc = per_channel(0.5, g.uniform(0.6, 1.4, (n, 3)).astype(f32))
        mul = g.uniform(0.6, 1.4, n).astype(f32)
        lin = per_channel(0.3, g.uniform(0.5, 2.2, (n, 3)).astype(f32))
        gray = g.uniform(0.0, 1.0, n).astype(f32)
        out = []
        for i in range(n):
            if not applied[i]:
                out.append(Program(False, int(seed[i]), ()))
                continue
            params = {1: (), 2: (float(sigma[i]),), 3: (float(enh[i, 0]),), 4: (float(enh[i, 1]),), 5: (float(enh[i, 2]),),
                      6: (float(enh[i, 3]),), 7: tuple(int(v) for v in add[i]), 8: tuple(int(v) for v in inv[i]),
                      9: tuple(float(v) for v in mul_pc[i]), 10: (float(mul[i]),) * 3, 11: (), 12: tuple(float(v) for v in lin[i]),
                      13: (float(gray[i]),)}
            out.append(Program(True, int(seed[i]), tuple((int(r) + 1, params[int(r) + 1]) for r in order[i] if fired[i, r])))
        return out


def program_to_records(programs):
    """Device encoding (include/picopose_hip.h): -> heads int32 (n, 4) = [op count, seed bits, applied, 0] and
    ops int32 (n, 13, 8) records, floats as their float32 bit patterns."""
    n = len(programs)
    heads = np.zeros((n, 4), np.int32)
    ops = np.zeros((n, MAX_OPS, OP_WORDS), np.int32)
    fbits = lambda v: int(np.float32(v).view(np.int32))  # noqa: E731
    for i, p in enumerate(programs):
        heads[i] = (len(p.ops), np.uint32(p.seed).view(np.int32), int(p.applied), 0)
        for k, (row, prm) in enumerate(p.ops):
            rec = ops[i, k]
            rec[0] = row
            if row == 2:
                r, q = gaussian_taps(prm[0])
                rec[1], rec[2:7], rec[7] = r, q, fbits(prm[0])
            elif row in (3, 4, 5, 6, 13):
                rec[1] = fbits(prm[0])
            elif row in (7, 8):
                rec[1:4] = prm
            elif row in (9, 10, 12):
                rec[1:4] = [fbits(v) for v in prm]
    return heads, ops


def records_to_program(heads, ops):
    """Inverse of program_to_records."""
    out = []
    for h, rows in zip(np.asarray(heads, np.int32), np.asarray(ops, np.int32)):
        fl = lambda w: float(np.int32(w).view(np.float32))  # noqa: E731
        prog = []
        for rec in rows[: int(h[0])]:
            row = int(rec[0])
            if row == 2:
                prm = (fl(rec[7]),)
            elif row in (3, 4, 5, 6, 13):
                prm = (fl(rec[1]),)
            elif row in (7, 8):
                prm = tuple(int(v) for v in rec[1:4])
            elif row in (9, 10, 12):
                prm = tuple(fl(v) for v in rec[1:4])
            else:
                prm = ()
            prog.append((row, prm))
        out.append(Program(bool(h[2]), int(np.int32(h[1]).view(np.uint32)), tuple(prog)))
    return out


def pass_starts(program):
    """Op index where each pass starts, then the op count: pass 0 crops, pass s > 0 starts at the s-th blur / sharpness /
    contrast op.  len - 1 = the passes the image takes (at most 4)."""
    return [0] + [k for k, (row, _) in enumerate(program.ops) if row in PASS_ROWS] + [len(program.ops)]


def nearest_template_views(R_opencv, template_poses, topk=5):
    """training_dataset.py:320-331 (`sample_template`) without the draw: the `topk` level-1 views whose OpenGL z axis lies
    nearest the query's.  template_poses (N, 4, 4) = utils/predefined_poses/obj_poses_level1.npy of the caller's checkout."""
    t = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]])
    query = np.matmul(t, np.asarray(R_opencv))[2, :3]
    tem = np.asarray(template_poses)[:, :3, :3]
    locations = np.matmul(np.tile(t, (tem.shape[0], 1, 1)), tem)[:, 2, :3]
    return np.argsort(np.linalg.norm(query - locations, axis=1))[:topk]


def _m_crop_resize(bbox, img_size):
    y1, y2, x1, x2 = bbox
    M_crop = np.array([[1, 0, -bbox[2]], [0, 1, -bbox[0]], [0, 0, 1]], dtype=np.float32)
    M_resize = np.array([[img_size / (y2 - y1), 0, 0], [0, img_size / (x2 - x1), 0], [0, 0, 1]], dtype=np.float32)
    return M_resize @ M_crop


def _fail(index, msg):
    raise ValueError(f"sample {index}: {msg}" if index is not None else msg)


def _prepare(s, ratio_real, ratio_tem, img_size, index=None):
    """Validates one decoded pair and computes its host-side values (training_dataset.py:173-316 without the pixels)."""
    rgb, mask, depth = np.asarray(s["rgb"]), np.asarray(s["mask"]), np.asarray(s["depth"])
    if rgb.ndim != 3 or rgb.shape[2] < 3 or rgb.dtype != np.uint8:
        _fail(index, f"rgb must be (H, W, 3) uint8, got {rgb.shape} {rgb.dtype}")
    H, W = rgb.shape[:2]
    if mask.shape != (H, W) or depth.shape != (H, W):
        _fail(index, f"mask {mask.shape} and depth {depth.shape} must match the frame {(H, W)}")
    if depth.dtype != np.uint16:
        _fail(index, f"depth must be uint16 (the PNG values), got {depth.dtype}")
    if mask.dtype not in (np.bool_, np.uint8) and (mask.min() < 0 or mask.max() > 255):
        _fail(index, "mask values must fit uint8")
    if not np.any(mask):
        _fail(index, "empty visible mask")
    bbox = get_bbox(mask > 0, ratio_real)
    y1, y2, x1, x2 = bbox
    if y1 < 0 or x1 < 0 or y2 > H or x2 > W:
        _fail(index, f"box {bbox} leaves the {H}x{W} frame")
    if np.count_nonzero(mask[y1:y2, x1:x2]) < MIN_MASK_PIXELS:
        _fail(index, f"fewer than {MIN_MASK_PIXELS} mask pixels in the crop")
    rgba, tdepth = np.asarray(s["tem_rgba"]), np.asarray(s["tem_depth"])
    if rgba.ndim != 3 or rgba.shape[2] != 4 or rgba.dtype != np.uint8:
        _fail(index, f"tem_rgba must be (H, W, 4) uint8, got {rgba.shape} {rgba.dtype}")
    if tdepth.shape != rgba.shape[:2] or tdepth.dtype != np.uint16:
        _fail(index, f"tem_depth must be uint16 {rgba.shape[:2]}, got {tdepth.shape} {tdepth.dtype}")
    alpha = rgba[..., 3]
    if not np.any(alpha):
        _fail(index, "empty template alpha")
    tbox = get_bbox(alpha > 0, ratio_tem)
    Ht, Wt = alpha.shape
    if tbox[0] < 0 or tbox[2] < 0 or tbox[1] > Ht or tbox[3] > Wt:
        _fail(index, f"template box {tbox} leaves the {Ht}x{Wt} frame")
    K, R, t = np.asarray(s["K"]), np.asarray(s["cam_R_m2c"]), np.asarray(s["cam_t_m2c"])
    tpose = np.array(s["tem_pose"])
    tK = np.asarray(s.get("templates_K", TEMPLATES_K))
    if K.size != 9 or R.size != 9 or t.size != 3 or tpose.shape != (4, 4) or tK.size != 9:
        _fail(index, "K, cam_R_m2c, templates_K need 9 values, cam_t_m2c 3, tem_pose (4, 4)")
    pose = np.eye(4)                                                    # training_dataset.py:190-192
    pose[:3, :3] = R.reshape(3, 3).astype(np.float32)
    pose[:3, 3] = t.reshape(3).astype(np.float32) / 1000.0
    tpose[:3, 3] = tpose[:3, 3] * 0.1 / 1000.0                          # :298
    return {"bbox": bbox, "tem_bbox": tbox, "M": _m_crop_resize(bbox, img_size), "tem_M": _m_crop_resize(tbox, img_size),
            "K": K.reshape(3, 3), "pose": pose, "tem_K": tK.reshape(3, 3), "tem_pose": tpose,
            "depth_scale": float(s["depth_scale"])}


def check_sample(sample, size_ratio=1.0, img_size=224):
    """The validity rule of read_data (training_dataset.py:184-185, 204-211, 270-271) plus the shapes the assembly needs:
    raises ValueError if the pair would be rejected (the caller's loader then draws another, as read_data's None does)."""
    _prepare(sample, size_ratio, size_ratio, img_size)


class AugmentPlan(NamedTuple):
    """Host side of one pp_augment_execute call: descriptors (n, IMG_WORDS), op records (n, 13, OP_WORDS), tiles (T, 4),
    pass_tiles (MAX_PASSES + 1), n_passes, n_buf (pixels of each ragged buffer)."""
    desc: np.ndarray
    ops: np.ndarray
    tiles: np.ndarray
    pass_tiles: list
    n_passes: int
    n_buf: int


def plan_augmentation(crops, programs):
    """crops: per image (frame buffer 0/1, pixel offset of the frame, frame width, (y1, y2, x1, x2), alpha mask mode);
    programs: one Program per image.  -> AugmentPlan (include/picopose_hip.h layout)."""
    n = len(crops)
    if len(programs) != n or n == 0:
        raise ValueError("one program per crop needed")
    heads, ops = program_to_records(programs)
    desc = np.zeros((n, IMG_WORDS), np.int64)
    for i, ((sel, off, fw, (y1, y2, x1, x2), alpha), prog) in enumerate(zip(crops, programs)):
        starts = pass_starts(prog)
        if len(starts) - 1 > MAX_PASSES:
            raise ValueError(f"program {i} needs more than {MAX_PASSES} passes")
        desc[i, :11] = (sel, off, fw, y1, x1, y2 - y1, x2 - x1, 0, heads[i, 1], i * MAX_OPS, len(starts) - 1)
        desc[i, 11:11 + len(starts)] = starts
        desc[i, 16] = int(alpha)
    hw = desc[:, 5] * desc[:, 6]
    desc[:, 7] = np.cumsum(hw) - hw
    tiles, pass_tiles = [], [0]
    for p in range(MAX_PASSES):
        ids = np.nonzero(desc[:, 10] > p)[0]
        ny, nx = (desc[ids, 5] + 15) // 16, (desc[ids, 6] + 15) // 16
        cnt = ny * nx
        local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        nxr = np.repeat(nx, cnt)
        tiles.append(np.stack([np.repeat(ids, cnt), local // nxr * 16, local % nxr * 16, np.zeros_like(local)], 1))
        pass_tiles.append(pass_tiles[-1] + len(local))
    n_passes = max(p for p in range(1, MAX_PASSES + 1) if pass_tiles[p] > pass_tiles[p - 1])
    if int(hw.sum()) >= 2 ** 31:
        raise ValueError("crops too large for 32-bit pixel offsets")
    return AugmentPlan(desc.astype(np.int32), ops, np.concatenate(tiles).astype(np.int32), pass_tiles, n_passes, int(hw.sum()))


def execute_augmentation(rgb0, mask0, rgba1, plan, device="cuda"):
    """Uploads the plan (one pinned buffer, one copy) and enqueues pp_augment_execute on the current stream.  rgb0 (..., 3) +
    mask0 (...) uint8: the real frames (buffer 0); rgba1 (..., 4) uint8: the template frames (buffer 1); device tensors.
    -> (buf0, buf1, descriptors on the device); image i's crop is
    buf[(nseg - 1) & 1][off : off + h w] with the layout of include/picopose_hip.h."""
    parts = [plan.desc.ravel(), plan.ops.ravel(), plan.tiles.ravel()]
    meta_h = torch.empty(sum(len(q) for q in parts), dtype=torch.int32, pin_memory=True)
    meta_h.numpy()[:] = np.concatenate(parts)
    meta = meta_h.to(device, non_blocking=True)
    n_img = len(plan.desc)
    d_desc = meta[:plan.desc.size]
    d_ops = meta[plan.desc.size:plan.desc.size + plan.ops.size]
    d_tiles = meta[plan.desc.size + plan.ops.size:]
    buf0 = torch.empty((plan.n_buf, 4), dtype=torch.uint8, device=device)
    buf1 = torch.empty((plan.n_buf, 4), dtype=torch.uint8, device=device)
    lsum = torch.empty(n_img, dtype=torch.int32, device=device)
    pt = (ctypes.c_int * (MAX_PASSES + 1))(*plan.pass_tiles)
    if rgb0.numel() != 3 * mask0.numel():
        raise ValueError("rgb0 and mask0 must hold the same frames")
    _lib.call("pp_augment_execute", rgb0, mask0, mask0.numel(), rgba1, rgba1.numel() // 4, d_desc, n_img, d_ops, n_img * MAX_OPS, d_tiles, pt,
              plan.n_passes, buf0, buf1, plan.n_buf, lsum)
    return buf0, buf1, d_desc


def assemble_training_batch(samples, img_size=224, augment_real=True, augment_tem=False, rgb_mask_flag=False, size_ratio=1.0,
                            generator=None, device="cuda", dilate_mask=False, programs=None):
    """Collated training batch of B decoded pairs -> end_points with the reference's keys (training_dataset.py:152-167):
    real_/tem_ full_depth (B,H,W), rgb (B,3,S,S), bbox (B,4), mask (B,S,S), M (B,3,3), K (B,3,3), pose (B,4,4), all fp32
    on `device`.  Each sample is a dict of decoded arrays:
      rgb (H,W,3) uint8 as load_im gives it, mask (H,W) visible mask (a dataset's mask_visib entry, or for a scene that has only
      scene_gt.json: picopose_amd.scene_gt.scene_gt_info(..., masks="visib")["mask_visib"], whose counts and visib_fract are also
      the instance filter of training_dataset.py:178), depth (H,W) uint16, depth_scale, K (3,3), cam_R_m2c (9),
      cam_t_m2c (3) in mm; tem_rgba (Ht,Wt,4) uint8, tem_depth (Ht,Wt) uint16 (PNG values), tem_pose (4,4) as stored
      (t in template units), templates_K (optional, the reference's by default).
    All real frames share one shape, all templates another.  `generator` (numpy Generator) draws the box ratios
    U(1, size_ratio) and the augmentation programs (ColorAugmentor); `programs` = (real, template) lists of Program
    overrides the draw of the programs.  Everything is enqueued on the current stream without a host synchronisation."""
    if dilate_mask:
        raise ValueError("dilate_mask=True is unsupported (the reference's default is False)")
    B = len(samples)
    if B == 0:
        raise ValueError("no samples")
    g = generator if generator is not None else np.random.default_rng()
    ratios = g.uniform(1.0, size_ratio, (2, B)) if size_ratio != 1.0 else np.ones((2, B))
    host = [_prepare(s, float(ratios[0, i]), float(ratios[1, i]), img_size, i) for i, s in enumerate(samples)]
    H, W = np.asarray(samples[0]["rgb"]).shape[:2]
    Ht, Wt = np.asarray(samples[0]["tem_rgba"]).shape[:2]
    for i, s in enumerate(samples):
        if np.asarray(s["rgb"]).shape[:2] != (H, W) or np.asarray(s["tem_rgba"]).shape[:2] != (Ht, Wt):
            _fail(i, f"frames must share one shape per view: {(H, W)} / {(Ht, Wt)} expected")
    if B * max(H * W, Ht * Wt) >= 2 ** 31:
        raise ValueError("batch too large for 32-bit pixel offsets")
    if programs is None:
        aug = ColorAugmentor(g)
        programs = (aug.sample(B) if augment_real else [EMPTY] * B, aug.sample(B) if augment_tem else [EMPTY] * B)
    progs = list(programs[0]) + list(programs[1])
    if len(progs) != 2 * B:
        raise ValueError("programs must hold B real and B template programs")

    crops = [(0, i * H * W, W, host[i]["bbox"], 0) for i in range(B)] + \
            [(1, i * Ht * Wt, Wt, host[i]["tem_bbox"], 1) for i in range(B)]
    plan = plan_augmentation(crops, progs)
    small = {k: np.stack([np.stack([np.asarray(hv[pre + k], np.float32) for hv in host]) for pre in ("", "tem_")])
             for k in ("bbox", "M", "K", "pose")}                      # each (2, B, ...): real, template
    scales = np.array([hv["depth_scale"] for hv in host], np.float32)
    f = np.concatenate([small[k].ravel() for k in ("bbox", "M", "K", "pose")] + [scales])
    f_h = torch.empty(len(f), dtype=torch.float32, pin_memory=True)
    f_h.numpy()[:] = f

    # ---- frames as decoded (real RGB + mask, template RGBA), depth uint16: each kind one pinned buffer and one copy
    fr_h = torch.empty((B, H, W, 3), dtype=torch.uint8, pin_memory=True)
    mk_h = torch.empty((B, H, W), dtype=torch.uint8, pin_memory=True)
    tf_h = torch.empty((B, Ht, Wt, 4), dtype=torch.uint8, pin_memory=True)
    dr_h = torch.empty((B, H, W), dtype=torch.int16, pin_memory=True)
    dt_h = torch.empty((B, Ht, Wt), dtype=torch.int16, pin_memory=True)
    fr, mk, tf, dr, dt = fr_h.numpy(), mk_h.numpy(), tf_h.numpy(), dr_h.numpy().view(np.uint16), dt_h.numpy().view(np.uint16)
    for b, s in enumerate(samples):
        fr[b] = np.asarray(s["rgb"])[..., :3]
        mk[b] = np.asarray(s["mask"])
        tf[b] = s["tem_rgba"]
        dr[b] = s["depth"]
        dt[b] = s["tem_depth"]
    rgb0, mask0, rgba1, d_f = (t.to(device, non_blocking=True) for t in (fr_h, mk_h, tf_h, f_h))
    dep_r, dep_t = dr_h.to(device, non_blocking=True), dt_h.to(device, non_blocking=True)
    buf0, buf1, d_desc = execute_augmentation(rgb0, mask0, rgba1, plan, device)
    n_img, S = 2 * B, img_size
    rgb = torch.empty((n_img, 3, S, S), dtype=torch.float32, device=device)
    msk = torch.empty((n_img, S, S), dtype=torch.float32, device=device)
    real_depth = torch.empty((B, H, W), dtype=torch.float32, device=device)
    tem_depth = torch.empty((B, Ht, Wt), dtype=torch.float32, device=device)
    mean, std = (ctypes.c_double * 3)(*CLIP_MEAN), (ctypes.c_double * 3)(*CLIP_STD)
    _lib.call("pp_augment_resize", buf0, buf1, plan.n_buf, d_desc, n_img, S, int(rgb_mask_flag), mean, std, rgb, msk)
    _lib.call("pp_depth_u16_scaled", dep_r, H * W, B, d_f[len(f) - B:], real_depth)
    _lib.call("pp_depth_u16_template", dep_t, B * Ht * Wt, tem_depth)
    ep = {"real_full_depth": real_depth, "tem_full_depth": tem_depth}
    o = 0
    for k, shape in (("bbox", (4,)), ("M", (3, 3)), ("K", (3, 3)), ("pose", (4, 4))):
        n = 2 * B * int(np.prod(shape))
        ep["real_" + k], ep["tem_" + k] = d_f[o:o + n].view(2, B, *shape).unbind(0)
        o += n
    ep["real_rgb"], ep["tem_rgb"] = rgb[:B], rgb[B:]
    ep["real_mask"], ep["tem_mask"] = msk[:B], msk[B:]
    return ep
