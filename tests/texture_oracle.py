"""Numpy statement of the texture contract of include/picopose_hip.h ("THE TEXTURE CONTRACT", T2-T5), written from that text and
built on render_oracle.Triangles for everything the raster contract already fixes (coverage, depth, the perspective weights).
The pyramid is integer arithmetic; every float operation is one float32 numpy operation in the stated order.  It is checked against
closed-form answers in tests/test_textured_bank_cpu.py; the GPU kernels are held to it bit for bit in tests/test_textured_bank_gpu.py."""
import numpy as np

import render_oracle as ro
from render_oracle import BG, F


def build_mips(texture):
    """T2: [level 0 (Ht, Wt, 3) uint8, level 1, ... down to (1, 1, 3)]."""
    lv = np.ascontiguousarray(np.asarray(texture, dtype=np.uint8))
    assert lv.ndim == 3 and lv.shape[2] == 3
    levels = [lv]
    while lv.shape[0] > 1 or lv.shape[1] > 1:
        h, w = lv.shape[:2]
        hd, wd = max(1, h >> 1), max(1, w >> 1)
        ya, yb = np.minimum(2 * np.arange(hd), h - 1), np.minimum(2 * np.arange(hd) + 1, h - 1)
        xa, xb = np.minimum(2 * np.arange(wd), w - 1), np.minimum(2 * np.arange(wd) + 1, w - 1)
        s = lv.astype(np.int64)
        lv = ((s[ya][:, xa] + s[ya][:, xb] + s[yb][:, xa] + s[yb][:, xb] + 2) >> 2).astype(np.uint8)
        levels.append(lv)
    return levels


def pack_mips(levels):
    """The device layout of T2: uchar4 texels {r, g, b, 255}, the levels back to back -> (n_texels, 4) uint8."""
    return np.concatenate([np.concatenate([lv.reshape(-1, 3), np.full((lv.shape[0] * lv.shape[1], 1), 255, np.uint8)], axis=1)
                           for lv in levels])


def expand_uv(uv, faces):
    """Per-vertex UVs (Nv, 2) -> per-corner UVs (Nf, 3, 2), the only layout the contract knows."""
    return np.ascontiguousarray(np.asarray(uv, dtype=F)[np.asarray(faces, dtype=np.int64)])


def face_levels(tri, faces, face_uv, Wt, Ht, n_levels):
    """T3 for every face of one view -> (Nf,) int64 (meaningful for the kept faces), and the corner UVs (Nf, 3, 2) in the order
    item 4 left the corners in."""
    fuv = np.asarray(face_uv, dtype=F)
    swapped = tri.ids[:, 1] != np.asarray(faces, dtype=np.int64)[:, 1]        # corners 1 and 2 were exchanged
    cuv = np.where(swapped[:, None, None], fuv[:, [0, 2, 1]], fuv)
    u0, v0, u1, v1, u2, v2 = cuv[:, 0, 0], cuv[:, 0, 1], cuv[:, 1, 0], cuv[:, 1, 1], cuv[:, 2, 0], cuv[:, 2, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        at = (np.abs(((u1 - u0) * (v2 - v0)) - ((v1 - v0) * (u2 - u0))) * F(Wt)) * F(Ht)
        lim = F(2) * (tri.area2.astype(F) / F(65536))
        level = np.zeros(len(fuv), dtype=np.int64)
        for l in range(n_levels - 1):
            go = (at > 0) & (level == l) & ~(at <= lim)
            level[go] += 1
            lim = np.where(go, lim * F(4), lim)
    return level, cuv


def sample(levels, level, u, v):
    """T4's wrap and T5 for samples with mip level `level` (n,) and interpolated coordinates u, v (n,) float32 -> (n, 3) uint8."""
    out = np.zeros((len(u), 3), dtype=np.uint8)
    u, v = u - np.floor(u), v - np.floor(v)
    for l in np.unique(level):
        m = level == l
        tex = levels[int(l)]
        Hl, Wl = tex.shape[:2]
        x, y = u[m] * F(Wl) - F(0.5), (F(1) - v[m]) * F(Hl) - F(0.5)
        xf, yf = np.floor(x), np.floor(y)
        fx, fy = x - xf, y - yf
        xa, xb = np.mod(xf.astype(np.int64), Wl), np.mod(xf.astype(np.int64) + 1, Wl)
        ya, yb = np.mod(yf.astype(np.int64), Hl), np.mod(yf.astype(np.int64) + 1, Hl)
        c00, c01, c10, c11 = (tex[a, b].astype(F) for a, b in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
        fx, fy = fx[:, None], fy[:, None]
        a = c00 + fx * (c01 - c00)
        b = c10 + fx * (c11 - c10)
        val = a + fy * (b - a)
        out[m] = np.clip(np.floor(val + F(0.5)), 0, 255).astype(np.uint8)
    return out


def render_view(vertices, faces, face_uv, texture, pose, K, H, W, near=1e-3, affine=False):
    """One view -> rgba (H,W,4) u8, depth_mm (H,W) u16, depth_m (H,W) f32, face_id (H,W) i32, level (H,W) i32 (-1 on background),
    near_count.  affine=True interpolates the UVs with the screen-space weights w_k / area2 instead of T4's perspective weights:
    NOT the contract, only the wrong answer a test of T4 must be able to tell from the right one."""
    tri = ro.Triangles(vertices, faces, pose, ro._k4(K), H, W, near)
    zbuf = np.full(H * W, BG, dtype=np.uint64)
    for pix, face, z in tri.fragments(H, W):                      # item 7
        key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | face.astype(np.uint64)
        np.minimum.at(zbuf, pix, key)
    rgba = np.zeros((H * W, 4), dtype=np.uint8)
    depth_mm = np.zeros(H * W, dtype=np.uint16)
    depth_m = np.zeros(H * W, dtype=F)
    face_id = np.full(H * W, -1, dtype=np.int32)
    level_map = np.full(H * W, -1, dtype=np.int32)
    hit = np.where(zbuf != BG)[0]
    if len(hit):
        levels = build_mips(texture)
        Ht, Wt = levels[0].shape[:2]
        face = (zbuf[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        z = (zbuf[hit] >> np.uint64(32)).astype(np.uint32).view(F)
        w, inside = tri.weights(face, hit % W, hit // W)
        assert inside.all()
        p, q = tri.depth_terms(face, w)
        if affine:
            a = tri.area2[face].astype(F)
            p, q = [w[k].astype(F) / a for k in range(3)], F(1)
        lvl, cuv = face_levels(tri, faces, face_uv, Wt, Ht, len(levels))
        c = cuv[face]
        u = ((p[0] * c[:, 0, 0] + p[1] * c[:, 1, 0]) + p[2] * c[:, 2, 0]) / q          # T4
        v = ((p[0] * c[:, 0, 1] + p[1] * c[:, 1, 1]) + p[2] * c[:, 2, 1]) / q
        rgba[hit, :3] = sample(levels, lvl[face], u, v)
        rgba[hit, 3] = 255
        depth_mm[hit] = np.minimum(np.rint(F(1000) * z), F(65535)).astype(np.uint16)     # item 8
        depth_m[hit] = z
        face_id[hit] = face.astype(np.int32)
        level_map[hit] = lvl[face].astype(np.int32)
    return {"rgba": rgba.reshape(H, W, 4), "depth_mm": depth_mm.reshape(H, W), "depth_m": depth_m.reshape(H, W),
            "face_id": face_id.reshape(H, W), "level": level_map.reshape(H, W), "near_count": tri.near_count}


def render(vertices, faces, face_uv, texture, poses, K, H, W, near=1e-3):
    """All views stacked; near_count summed."""
    views = [render_view(vertices, faces, face_uv, texture, p, K, H, W, near) for p in poses]
    out = {k: np.stack([v[k] for v in views]) for k in ("rgba", "depth_mm", "depth_m", "face_id", "level")}
    out["near_count"] = sum(v["near_count"] for v in views)
    return out


# ---- test scenes (generated, never committed) ------------------------------------------------------------------------------------
K_SMALL = np.array([[512.0, 0, 32.0], [0, 512.0, 24.0], [0, 0, 1.0]])        # with Zc = 2: x = 256 X + 32, exact for dyadic X
Z_SMALL = 2.0
FRAME = (48, 64)


def pose(R=np.eye(3), t=(0, 0, Z_SMALL)):
    P = np.eye(4, dtype=np.float32)
    P[:3, :3], P[:3, 3] = R, t
    return P


def screen_quad(x0, y0, wpx, hpx):
    """A fronto-parallel quad that covers exactly the pixels x0 <= x < x0 + wpx, y0 <= y < y0 + hpx of a K_SMALL frame at depth
    Z_SMALL: its edges sit half a pixel outside the first / last pixel centre, on exact 1/256 px positions.  Vertices TL, TR, BL, BR
    with the whole texture mapped upright: (u, v) = (0, 1), (1, 1), (0, 0), (1, 0).  -> vertices, faces, per-vertex uv."""
    xs, ys = (x0 - 0.5, x0 + wpx - 0.5), (y0 - 0.5, y0 + hpx - 0.5)
    v = np.array([[(x - 32) / 256, (y - 24) / 256, 0.0] for y in ys for x in xs], dtype=np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2]], dtype=np.int32)
    uv = np.array([[0, 1], [1, 1], [0, 0], [1, 0]], dtype=np.float32)
    return v, f, uv


def random_texture(Wt, Ht, seed):
    return np.random.default_rng(seed).integers(0, 256, (Ht, Wt, 3)).astype(np.uint8)
