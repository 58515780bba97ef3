"""numpy restatement of "THE SCENE COMPOSITE" of include/picopose_hip.h (csrc/pp_synth.hip): the per-pixel winner over an image's
layers, the colour / 16-bit depth / instance outputs, the per-layer counts, boxes and masks, the three background modes (the lattice in
integers, with the counter hash of tests/train_batch_oracle.py) and the depth quantiser.  float32 with one rounding per operation."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_batch_oracle import hash3  # noqa: E402

F = np.float32
BG_WORDS = 4


def lattice(seed, s, H, W):
    """Mode 2 -> (H, W, 3) uint8: cell 2^s, node (u, v) = bytes 0..2 of h(seed, u, v), integer bilinear blend."""
    S = 1 << s
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    gx, gy, fx, fy = x >> s, y >> s, x & (S - 1), y & (S - 1)
    seed = np.uint32(int(seed) & 0xFFFFFFFF)

    def node(u, v):
        return hash3(seed, u.astype(np.uint32), v.astype(np.uint32)).astype(np.int64)

    n00, n10, n01, n11 = node(gx, gy), node(gx + 1, gy), node(gx, gy + 1), node(gx + 1, gy + 1)
    out = np.zeros((H, W, 3), np.uint8)
    for c in range(3):
        b = [(n >> (8 * c)) & 255 for n in (n00, n10, n01, n11)]
        v = b[0] * (S - fx) * (S - fy) + b[1] * fx * (S - fy) + b[2] * (S - fx) * fy + b[3] * fx * fy
        out[..., c] = (v + (1 << (2 * s - 1))) >> (2 * s)
    return out


def background(desc, bg_image, H, W):
    """One image's background (H, W, 3) uint8 from its descriptor {mode, a, b, 0}."""
    mode, a, b = int(desc[0]), int(desc[1]), int(desc[2])
    if mode == 0:
        a &= 0xFFFFFFFF
        return np.broadcast_to(np.array([a & 255, (a >> 8) & 255, (a >> 16) & 255], np.uint8), (H, W, 3)).copy()
    if mode == 1:
        return np.asarray(bg_image, np.uint8).copy()
    return lattice(a, b, H, W)


def quantize_scene_depth(z, depth_scale):
    """min(65535, rintf((1000.0f * Z) / depth_scale)) in float32, for Z > 0."""
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.rint((F(1000.0) * z.astype(F)).astype(F) / F(depth_scale))
    return np.minimum(q, F(65535)).astype(np.uint16)


def depth_quantize_u16(depth_m, units_per_metre):
    """pp_depth_quantize_u16: Z > 0 ? min(65535, rintf(units * Z)) : 0."""
    z = np.asarray(depth_m, F)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.minimum(np.rint((F(units_per_metre) * z).astype(F)), F(65535))
        cover = z > 0
    return np.where(cover, np.where(cover, q, 0), 0).astype(np.uint16)


def composite(layers_rgba, layers_depth, layer_off, backgrounds, depth_scale, bg_images=None):
    """-> {"rgb" (n, H, W, 3) u8, "depth" (n, H, W) u16, "instance" (n, H, W) i32, "counts" (L, 2) i32, "boxes" (L, 4) i32,
    "mask_visib" (L, H, W) u8}.  layers_rgba (L, H, W, 4), layers_depth (L, H, W) f32, layer_off (n + 1), backgrounds (n, 4) int,
    depth_scale (n,), bg_images (n, H, W, 3) or None.  H, W come from `shape` of the layers or, with L = 0, of bg_images."""
    layers_depth = np.asarray(layers_depth, F)
    L, H, W = layers_depth.shape
    n = len(layer_off) - 1
    rgb = np.zeros((n, H, W, 3), np.uint8)
    depth = np.zeros((n, H, W), np.uint16)
    inst = np.full((n, H, W), -1, np.int32)
    counts = np.zeros((L, 2), np.int32)
    boxes = np.tile(np.array([0, 0, -1, -1], np.int32), (L, 1))
    mask = np.zeros((L, H, W), np.uint8)
    BG = np.uint64(0xFFFFFFFFFFFFFFFF)
    for i in range(n):
        key = np.full((H, W), BG, np.uint64)
        for l in range(int(layer_off[i]), int(layer_off[i + 1])):
            z = layers_depth[l]
            with np.errstate(invalid="ignore"):
                cover = z > 0                                          # NaN, negatives and +-0 do not cover
            counts[l, 0] = int(cover.sum())
            k = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(l)
            key = np.where(cover, np.minimum(key, k), key)
        won = key != BG
        win_l = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
        win_z = (key >> np.uint64(32)).astype(np.uint32).view(F)
        rgb[i] = background(backgrounds[i], None if bg_images is None else bg_images[i], H, W)
        if won.any():
            yy, xx = np.nonzero(won)
            rgb[i][yy, xx] = layers_rgba[win_l[yy, xx], yy, xx, :3]
            depth[i][yy, xx] = quantize_scene_depth(win_z[yy, xx], depth_scale[i])
            inst[i][yy, xx] = win_l[yy, xx].astype(np.int32)
        for l in range(int(layer_off[i]), int(layer_off[i + 1])):
            m = won & (win_l == l)
            mask[l] = np.where(m, 255, 0)
            counts[l, 1] = int(m.sum())
            if m.any():
                yy, xx = np.nonzero(m)
                boxes[l] = (xx.min(), yy.min(), xx.max(), yy.max())
    return {"rgb": rgb, "depth": depth, "instance": inst, "counts": counts, "boxes": boxes, "mask_visib": mask}
