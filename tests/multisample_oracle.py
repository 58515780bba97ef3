"""Numpy statement of the multisample contract of include/picopose_hip.h ("THE MULTISAMPLE CONTRACT", M1-M5), written from that
text and built on render_oracle / texture_oracle / shading_oracle for everything the raster, texture and shading contracts already
fix.  A plane is render_oracle.Triangles with the snapped coordinates moved back by the plane's offset and the sample boxes
recomputed (M2); the colour of a covered sample is the existing arithmetic evaluated with that plane's weights (M3); the resolve is
integer (M4); the geometry outputs are the centre plane's (M5).  It is checked against closed-form answers in
tests/test_multisample_cpu.py; the GPU kernels are held to it bit for bit in tests/test_multisample_gpu.py."""
import numpy as np

import render_oracle as ro
import shading_oracle as so
import texture_oracle as to
from render_oracle import BG, F, SUB

CENTRE = (0, 0)
OFFSETS = ((-32, -96), (96, -32), (-96, 32), (32, 96))            # M1: the rotated grid in 1/16 pixel, times 16
ALPHAS = (0, 64, 128, 191, 255)                                   # (255 n + 2) >> 2 for n = 0 .. 4 covered samples


class PlaneTriangles(ro.Triangles):
    """M2: the triangles of one view as the plane with offset (ox, oy) sees them — snapped coordinates (xs - ox, ys - oy), the
    sample boxes recomputed from them; area2, the winding exchange, the vertex order and 1 / Zc are those of the centre."""

    def __init__(self, vertices, faces, pose, K4, H, W, near, offset):
        super().__init__(vertices, faces, pose, K4, H, W, near)
        ok = ro.project(vertices, pose, *K4, near)[3]
        near_tri = ~ok[np.asarray(faces, dtype=np.int64)].all(axis=1)
        assert int(near_tri.sum()) == self.near_count
        self.x = self.x - int(offset[0])
        self.y = self.y - int(offset[1])
        self.bx0 = np.maximum((self.x.min(axis=1) + SUB - 1) >> 8, 0)
        self.bx1 = np.minimum(self.x.max(axis=1) >> 8, W - 1)
        self.by0 = np.maximum((self.y.min(axis=1) + SUB - 1) >> 8, 0)
        self.by1 = np.minimum(self.y.max(axis=1) >> 8, H - 1)
        self.keep = ~near_tri & (self.area2 != 0) & (self.bx0 <= self.bx1) & (self.by0 <= self.by1)


def vertex_colour(colors):
    """Item 6's colour as a per-sample colour function."""
    colors = np.asarray(colors)

    def fn(tri, face, p, q):
        col = [colors[tri.ids[face, k]].astype(F) for k in range(3)]
        out = np.zeros((len(face), 3), dtype=np.uint8)
        for ch in range(3):
            val = np.floor(((p[0] * col[0][:, ch] + p[1] * col[1][:, ch]) + p[2] * col[2][:, ch]) / q + F(0.5))
            out[:, ch] = np.clip(val, 0, 255).astype(np.uint8)
        return out
    return fn


def textured(faces, face_uv, texture):
    """T3-T5 as a per-sample colour function (the level per (plane, face) from the plane's triangles: area2 does not move)."""
    levels = to.build_mips(texture)
    Ht, Wt = levels[0].shape[:2]

    def fn(tri, face, p, q):
        lvl, cuv = to.face_levels(tri, faces, face_uv, Wt, Ht, len(levels))
        c = cuv[face]
        u = ((p[0] * c[:, 0, 0] + p[1] * c[:, 1, 0]) + p[2] * c[:, 2, 0]) / q
        v = ((p[0] * c[:, 0, 1] + p[1] * c[:, 1, 1]) + p[2] * c[:, 2, 1]) / q
        return to.sample(levels, lvl[face], u, v)
    return fn


def constant(rgb):
    return lambda tri, face, p, q: np.tile(np.asarray(rgb, dtype=np.uint8), (len(face), 1))


def lit(base_fn, pose, vertices, lights4, ambient, normals=None, tone=None):
    """S2-S6 around a base colour function, for the view with `pose`."""
    def fn(tri, face, p, q):
        return so.shade(tri, pose, vertices, face, p, q, base_fn(tri, face, p, q), lights4, ambient, normals, tone)[0]
    return fn


def mesh_colour(mesh, pose, shading=None):
    """The colour function of `mesh` ({"vertices", "faces"} + "colors" or "texture" and "face_uv") for the view with `pose`.
    shading: None or {"lights4", "ambient", "normals" (None = flat), "base_color" (None), "tone" (None)}."""
    if shading is not None and shading.get("base_color") is not None:
        base = constant(shading["base_color"])
    elif mesh.get("texture") is not None:
        base = textured(mesh["faces"], mesh["face_uv"], mesh["texture"])
    else:
        base = vertex_colour(mesh["colors"])
    if shading is None:
        return base
    return lit(base, pose, mesh["vertices"], shading["lights4"], shading["ambient"], shading.get("normals"), shading.get("tone"))


def render_plane(vertices, faces, pose, K, H, W, offset, colour_fn=None, near=1e-3):
    """One plane of one view -> {"zbuf" (H W,) uint64, "rgba" (H, W, 4) uint8 (when colour_fn is given), "near_count"}."""
    tri = PlaneTriangles(vertices, faces, pose, ro._k4(K), H, W, near, offset)
    zbuf = np.full(H * W, BG, dtype=np.uint64)
    for pix, face, z in tri.fragments(H, W):                      # item 7
        key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | face.astype(np.uint64)
        np.minimum.at(zbuf, pix, key)
    out = {"zbuf": zbuf, "near_count": tri.near_count}
    if colour_fn is not None:
        rgba = np.zeros((H * W, 4), dtype=np.uint8)
        hit = np.where(zbuf != BG)[0]
        if len(hit):
            face = (zbuf[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            w, inside = tri.weights(face, hit % W, hit // W)
            assert inside.all()
            p, q = tri.depth_terms(face, w)
            rgba[hit, :3] = colour_fn(tri, face, p, q)
            rgba[hit, 3] = 255
        out["rgba"] = rgba.reshape(H, W, 4)
    return out


def geometry(zbuf, H, W):
    """Item 8 from the z-buffer words of the centre plane (M5) -> depth_mm, depth_m, face_id."""
    depth_mm = np.zeros(H * W, dtype=np.uint16)
    depth_m = np.zeros(H * W, dtype=F)
    face_id = np.full(H * W, -1, dtype=np.int32)
    hit = np.where(zbuf != BG)[0]
    z = (zbuf[hit] >> np.uint64(32)).astype(np.uint32).view(F)
    depth_mm[hit] = np.minimum(np.rint(F(1000) * z), F(65535)).astype(np.uint16)
    depth_m[hit] = z
    face_id[hit] = (zbuf[hit] & np.uint64(0xFFFFFFFF)).astype(np.int32)
    return depth_mm.reshape(H, W), depth_m.reshape(H, W), face_id.reshape(H, W)


def resolve(planes):
    """M4: (sum of the four sample planes + 2) >> 2 per channel."""
    acc = np.zeros(planes[0].shape, dtype=np.int64)
    for pl in planes:
        acc += pl
    return ((acc + 2) >> 2).astype(np.uint8)


def render_view(mesh, pose, K, H, W, shading=None, near=1e-3):
    """One multisampled view of `mesh` -> rgba (H,W,4) u8 (M3, M4), depth_mm, depth_m, face_id (M5), near_count (once, M2),
    "centre_rgba" (the centre plane's colour: the single-sample render) and "covered" (H,W) the number of covered samples."""
    v, f = mesh["vertices"], mesh["faces"]
    fn = mesh_colour(mesh, pose, shading)
    centre = render_plane(v, f, pose, K, H, W, CENTRE, fn, near)
    planes = [render_plane(v, f, pose, K, H, W, o, fn, near)["rgba"] for o in OFFSETS]
    depth_mm, depth_m, face_id = geometry(centre["zbuf"], H, W)
    return {"rgba": resolve(planes), "depth_mm": depth_mm, "depth_m": depth_m, "face_id": face_id, "near_count": centre["near_count"],
            "centre_rgba": centre["rgba"], "covered": sum((pl[..., 3] == 255).astype(np.int64) for pl in planes)}


def render(mesh, poses, K, H, W, shading=None, near=1e-3):
    """All views stacked; near_count summed."""
    views = [render_view(mesh, p, K, H, W, shading, near) for p in poses]
    out = {k: np.stack([x[k] for x in views]) for k in ("rgba", "depth_mm", "depth_m", "face_id", "centre_rgba", "covered")}
    out["near_count"] = sum(x["near_count"] for x in views)
    return out


def edge_stats(view):
    """The three counts a GPU scene must show (per view): partially covered pixels, alpha > 0 with an empty centre, centre hit
    with alpha < 255 (M5's two kinds)."""
    a, hit = view["rgba"][..., 3], view["face_id"] >= 0
    return int(((a > 0) & (a < 255)).sum()), int(((a > 0) & ~hit).sum()), int((hit & (a < 255)).sum())


# ---- test scenes (generated, never committed) ------------------------------------------------------------------------------------
K_TEST = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1.0]])
FRAME = (48, 64)


def random_poses(n, distance, seed):
    """n object -> camera poses with a random rotation and t = (0, 0, distance)."""
    rng = np.random.default_rng(seed)
    P = np.zeros((n, 4, 4), dtype=np.float32)
    for k in range(n):
        Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
        Q = Q * np.sign(np.diag(R))
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        P[k, :3, :3], P[k, :3, 3], P[k, 3, 3] = Q, (0, 0, distance), 1
    return P


def textured_icosphere(seed):
    """The textured scene of tests/test_textured_bank_gpu.py: a 320-triangle icosphere, a random 12 x 6 texture, random per-corner
    UVs that leave [0, 1] and are scaled per face so that one frame shows several mip levels."""
    m = ro.icosphere(2, 0.5)
    rng = np.random.default_rng(seed)
    nf = len(m["faces"])
    fuv = rng.uniform(-0.5, 0.5, (nf, 3, 2)) * 2.0 ** (np.arange(nf) % 6 - 2)[:, None, None] + rng.uniform(-1.5, 1.5, (nf, 1, 2))
    return {"vertices": m["vertices"], "faces": m["faces"], "face_uv": fuv.astype(np.float32), "texture": to.random_texture(12, 6, seed)}


def scenes():
    """The scenes of the GPU tests -> {name: (mesh, poses (V,4,4) f32, K, (H, W), shading for render_views or None)}; vertices
    and translations in metres (units="m")."""
    cube = ro.cube(0.4)
    ico = ro.icosphere(2, 0.5)
    rng = np.random.default_rng(8)
    smooth = dict(ico, normals=rng.normal(size=ico["vertices"].shape).astype(np.float32))       # normals of its own, not unit length
    lights = {"lights": np.array([[0.6, -0.8, 0.1], [-1.0, 0.5, 0.3], [0.0, 0.0, 4.0]]), "intensity": np.array([0.9, 0.6, 0.5])}
    K90 = np.array([[90.0, 0, 31.5], [0, 88.0, 23.5], [0, 0, 1.0]])
    diameter = float(np.linalg.norm(np.ptp(cube["vertices"].astype(np.float64), axis=0) * 2))
    return {
        "cube": (ro.cube(0.06), random_poses(4, 0.4, 3), K_TEST, FRAME, None),
        "icosphere": (ro.icosphere(2, 0.1), random_poses(4, 0.4, 4), K_TEST, FRAME, None),
        "textured": (textured_icosphere(21), random_poses(3, 1.6, 5), K_TEST, (47, 61), None),
        "tless": ({"vertices": cube["vertices"], "faces": cube["faces"]}, random_poses(3, diameter, 6), K90, FRAME, "tless"),
        "smooth_tone": (smooth, random_poses(3, 1.6, 7), K_TEST, FRAME, dict(lights, ambient=0.25, normals="smooth", tone="srgb")),
    }


def oracle_shading(shading, mesh):
    """render_views' `shading` -> mesh_colour's dict, through the package's own (host-side, numpy) parser."""
    if shading is None:
        return None
    from picopose_amd.provider import template_bank as tb

    diameter = float(np.linalg.norm(np.ptp(np.asarray(mesh["vertices"], dtype=np.float64), axis=0) * 2))
    lights4, ambient, smooth, base, tone = tb._parse_shading(shading, diameter)
    return {"lights4": lights4, "ambient": ambient, "normals": np.asarray(mesh["normals"], dtype=F) if smooth else None,
            "base_color": base, "tone": tone}


# the exact frame of texture_oracle: with Zc = 2 a vertex at X lands on pixel 256 X + 32, so sub-pixel positions are chosen exactly
K_EXACT, Z_EXACT = to.K_SMALL, to.Z_SMALL


def at_subpixels(xy_sub, z=0.0):
    """Object-space vertices (n, 3) float32 that the identity pose at Z_EXACT snaps onto the sub-pixel positions xy_sub (n, 2)."""
    xy = np.asarray(xy_sub, dtype=np.float64)
    return np.stack([(xy[:, 0] / 256 - 32) / 256, (xy[:, 1] / 256 - 24) / 256, np.full(len(xy), z)], axis=1).astype(np.float32)


def edge_scene():
    """One mesh, two views, a 48 x 64 frame.  Faces 0-3: a cross of two bars that leaves the frame on all four sides.  Face 4: a
    triangle with a vertex behind the camera in view 0 (dropped at the near plane).  Faces 5 ...: 72 triangles of less than a
    pixel's area at random sub-pixel positions in the four free quadrants, and a sliver through four sample positions.  View 0: the identity pose at Z_EXACT.  View 1: the
    same at 30 times the distance, where the bars are 63 and 73 sub-pixels thick against a spacing of 64 between sample rows and
    columns: the horizontal bar holds at most one sample of a pixel, the vertical one or two, so partial pixels only.
    -> mesh, poses (2,4,4) f32, K, (H, W)"""
    rng = np.random.default_rng(12)
    bars = [(-2600, 5200, 19000, 7100), (7200, -2500, 9400, 14800)]                   # x0, y0, x1, y1 in sub-pixels
    xy, faces = [], []
    for x0, y0, x1, y1 in bars:
        n = len(xy)
        xy += [(x0, y0), (x1, y0), (x0, y1), (x1, y1)]
        faces += [[n, n + 1, n + 3], [n, n + 3, n + 2]]
    verts = [at_subpixels(xy)]
    n = len(xy)
    verts.append(np.array([[0.3, 0.3, -2.5], [0.31, 0.3, -2.5], [0.3, 0.31, 0.0]], dtype=np.float32))       # Zc = -0.5 in view 0
    faces.append([n, n + 1, n + 2])
    n += 3
    tiny = []
    for qx, qy in ((2, 2), (40, 2), (2, 30), (40, 30)):                               # quadrant origins in pixels: 6 x 3 cells of 3 x 5
        for cx in range(6):
            for cy in range(3):
                o = np.array([(qx + 3 * cx + 1) * 256, (qy + 5 * cy + 2) * 256])
                while True:
                    t = o + rng.integers(-200, 200, (3, 2))
                    a2 = abs((t[1, 0] - t[0, 0]) * (t[2, 1] - t[0, 1]) - (t[1, 1] - t[0, 1]) * (t[2, 0] - t[0, 0]))
                    if 0 < a2 < 2 * 65536:                                            # less than a pixel's area
                        break
                tiny.append(t)
    # a sliver along the line x + y = 128 of pixel (60, 44), on which four sample positions lie: (288, -160), (224, -96), (32, 96), (-32, 160)
    tiny.append(np.array([60 * 256, 44 * 256]) + np.array([(310, -190), (318, -182), (-60, 188)]))
    for t in tiny:
        faces.append([n, n + 1, n + 2])
        n += 3
    verts.append(at_subpixels(np.concatenate(tiny)))
    v = np.concatenate(verts)
    mesh = {"vertices": v, "faces": np.array(faces, dtype=np.int32), "colors": rng.integers(30, 256, (len(v), 3)).astype(np.uint8)}
    poses = np.stack([to.pose(), to.pose(t=(0, 0, 30 * Z_EXACT))]).astype(np.float32)
    return mesh, poses, K_EXACT, to.FRAME


def speck_scene():
    """A cube that render_templates places at its diameter under a focal length of three pixels: about a pixel wide, centred on
    the corner that pixels (32 .. 33, 24 .. 25) share — it covers one sample of each of the four (alpha 64 everywhere it is seen).
    -> mesh, view_poses (1,4,4), K, (H, W)"""
    c = ro.cube(0.4)
    K = np.array([[3.0, 0, 32.5], [0, 3.0, 24.5], [0, 0, 1.0]])
    return {"vertices": c["vertices"], "faces": c["faces"], "colors": c["colors"]}, np.eye(4)[None], K, FRAME


def bank_scene():
    """The scene of the bank test: the coloured cube at 96 x 128 under a principal point off the pixel grid, so that the square
    crop window grows under multisampling in some of the test's views and not in others -> mesh, K, (H, W)."""
    return ro.cube(0.4), np.array([[118.0, 0, 64.4], [0, 118.0, 48.3], [0, 0, 1.0]]), (96, 128)
