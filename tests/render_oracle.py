"""Numpy statement of the raster contract of include/picopose_hip.h ("THE RASTER CONTRACT", items 1-8), written from that text:
float32 vertex arithmetic in the stated order (numpy rounds every float32 operation once and never contracts), int64 edge
functions, the top-left fill rule, the depth / face-index tie rule and the two roundings.  It is checked against closed-form
answers in tests/test_template_bank_cpu.py; the GPU rasteriser is held to it bit for bit in tests/test_template_bank_gpu.py.

Only the evaluation ORDER over samples differs from a naive loop: triangles are grouped by the size of their sample box and each
group is evaluated on a dense grid (every sample of every box is tested, as the contract says), so the reference views of a
20 k-triangle mesh take seconds."""
import numpy as np

F = np.float32
SUB = 256
SNAP = 2 ** 28
BG = np.uint64(0xFFFFFFFFFFFFFFFF)


def project(vertices, pose, fx, fy, cx, cy, near):
    """Items 1-3 for every vertex -> xs, ys (int64), 1 / Zc (float32), Zc > near."""
    P, v = np.asarray(pose, dtype=F), np.asarray(vertices, dtype=F)
    X, Y, Z = v[:, 0], v[:, 1], v[:, 2]

    def row(r):
        return ((P[r, 0] * X + P[r, 1] * Y) + P[r, 2] * Z) + P[r, 3]

    xc, yc, zc = row(0), row(1), row(2)
    ok = zc > F(near)
    zs = np.where(ok, zc, F(1))
    u = (F(fx) * xc) / zs + F(cx)
    w = (F(fy) * yc) / zs + F(cy)
    snap = lambda a: np.rint(np.clip(a * F(SUB), -F(SNAP), F(SNAP))).astype(np.int64)  # noqa: E731
    return snap(u), snap(w), F(1) / zs, ok


class Triangles:
    """Items 1-4 for every face of one view: ordered vertices, area2 > 0, the clipped sample box; `keep` = the faces that can
    cover a sample, `near_count` = the faces dropped at the near plane."""

    def __init__(self, vertices, faces, pose, K4, H, W, near):
        xs, ys, iz, ok = project(vertices, pose, *K4, near)
        f = np.asarray(faces, dtype=np.int64)
        near_tri = ~ok[f].all(axis=1)
        self.near_count = int(near_tri.sum())
        x, y, z, ids = xs[f], ys[f], iz[f], f.copy()
        area2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
        flip = area2 < 0
        for a in (x, y, z, ids):
            a[flip] = a[flip][:, [0, 2, 1]]
        self.x, self.y, self.iz, self.ids, self.area2 = x, y, z, ids, np.abs(area2)
        self.bx0 = np.maximum((x.min(axis=1) + SUB - 1) >> 8, 0)
        self.bx1 = np.minimum(x.max(axis=1) >> 8, W - 1)
        self.by0 = np.maximum((y.min(axis=1) + SUB - 1) >> 8, 0)
        self.by1 = np.minimum(y.max(axis=1) >> 8, H - 1)
        self.keep = ~near_tri & (area2 != 0) & (self.bx0 <= self.bx1) & (self.by0 <= self.by1)

    def weights(self, t, px, py):
        """Item 5 for triangles t (n,) at samples px, py (broadcastable to (n, ...)) -> w (3, n, ...) int64, covered mask."""
        ex = (Ellipsis,) + (None,) * (np.ndim(px) - 1)
        w, inside = [], True
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            xa, ya = self.x[t, a][ex], self.y[t, a][ex]
            dx, dy = self.x[t, b][ex] - xa, self.y[t, b][ex] - ya
            wk = dx * (py * SUB - ya) - dy * (px * SUB - xa)
            owns = (dy < 0) | ((dy == 0) & (dx > 0))
            inside = inside & ((wk > 0) | ((wk == 0) & owns))
            w.append(wk)
        return w, inside

    def depth_terms(self, t, w):
        """Item 6: p_k and q for triangle indices t and integer weights w (each shaped like t)."""
        a = self.area2[t].astype(F)
        p = [(w[k].astype(F) / a) * self.iz[t, k] for k in range(3)]
        return p, (p[0] + p[1]) + p[2]

    def fragments(self, H, W):
        """Yield (sample index y W + x, face, Z float32) for every covered sample of every kept triangle."""
        idx = np.where(self.keep)[0]
        bw, bh = self.bx1[idx] - self.bx0[idx] + 1, self.by1[idx] - self.by0[idx] + 1
        size = np.maximum(bw, bh)
        cls = np.ceil(np.log2(np.maximum(size, 1))).astype(int)
        for c in np.unique(cls):
            group = idx[cls == c]
            n = 1 << int(c)
            if n <= 32:                                           # dense n x n grid per triangle, in batches
                step = max(1, (1 << 22) // (n * n))
                off = np.arange(n, dtype=np.int64)
                for s in range(0, len(group), step):
                    t = group[s:s + step]
                    px = self.bx0[t][:, None, None] + off[None, None, :]
                    py = self.by0[t][:, None, None] + off[None, :, None]
                    w, inside = self.weights(t, px, py)
                    inside = inside & (px <= self.bx1[t][:, None, None]) & (py <= self.by1[t][:, None, None])
                    k, j, i = np.nonzero(inside)
                    tt = t[k]
                    _, q = self.depth_terms(tt, [wk[k, j, i] for wk in w])
                    yield (py[k, j, 0] * W + px[k, 0, i]), tt, F(1) / q
            else:                                                 # one triangle at a time over its own box
                for t1 in group:
                    t = np.array([t1])
                    px = np.arange(self.bx0[t1], self.bx1[t1] + 1, dtype=np.int64)[None, None, :]
                    py = np.arange(self.by0[t1], self.by1[t1] + 1, dtype=np.int64)[None, :, None]
                    w, inside = self.weights(t, px, py)
                    _, j, i = np.nonzero(inside)
                    tt = np.full(len(j), t1)
                    _, q = self.depth_terms(tt, [wk[0, j, i] for wk in w])
                    yield (py[0, j, 0] * W + px[0, 0, i]), tt, F(1) / q


def _k4(K):
    K = np.asarray(K, dtype=np.float64)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def coverage_counts(vertices, faces, pose, K, H, W, near=1e-3):
    """How many triangles cover each sample (no depth test) -> (H, W) int64."""
    tri = Triangles(vertices, faces, pose, _k4(K), H, W, near)
    cnt = np.zeros(H * W, dtype=np.int64)
    for pix, _, _ in tri.fragments(H, W):
        np.add.at(cnt, pix, 1)
    return cnt.reshape(H, W)


def render_view(vertices, faces, colors, pose, K, H, W, near=1e-3):
    """One view -> rgba (H,W,4) u8, depth_mm (H,W) u16, depth_m (H,W) f32, face_id (H,W) i32, near_count."""
    tri = Triangles(vertices, faces, pose, _k4(K), H, W, near)
    zbuf = np.full(H * W, BG, dtype=np.uint64)
    for pix, face, z in tri.fragments(H, W):                      # item 7
        key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | face.astype(np.uint64)
        np.minimum.at(zbuf, pix, key)
    rgba = np.zeros((H * W, 4), dtype=np.uint8)
    depth_mm = np.zeros(H * W, dtype=np.uint16)
    depth_m = np.zeros(H * W, dtype=F)
    face_id = np.full(H * W, -1, dtype=np.int32)
    hit = np.where(zbuf != BG)[0]
    if len(hit):
        face = (zbuf[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        z = (zbuf[hit] >> np.uint64(32)).astype(np.uint32).view(F)
        w, inside = tri.weights(face, hit % W, hit // W)
        assert inside.all()
        p, q = tri.depth_terms(face, w)
        col = [np.asarray(colors)[tri.ids[face, k]].astype(F) for k in range(3)]
        for ch in range(3):                                       # item 6
            val = np.floor(((p[0] * col[0][:, ch] + p[1] * col[1][:, ch]) + p[2] * col[2][:, ch]) / q + F(0.5))
            rgba[hit, ch] = np.clip(val, 0, 255).astype(np.uint8)
        rgba[hit, 3] = 255
        depth_mm[hit] = np.minimum(np.rint(F(1000) * z), F(65535)).astype(np.uint16)     # item 8
        depth_m[hit] = z
        face_id[hit] = face.astype(np.int32)
    return {"rgba": rgba.reshape(H, W, 4), "depth_mm": depth_mm.reshape(H, W), "depth_m": depth_m.reshape(H, W),
            "face_id": face_id.reshape(H, W), "near_count": tri.near_count}


def render(vertices, faces, colors, poses, K, H, W, near=1e-3):
    """All views stacked; near_count summed."""
    views = [render_view(vertices, faces, colors, p, K, H, W, near) for p in poses]
    out = {k: np.stack([v[k] for v in views]) for k in ("rgba", "depth_mm", "depth_m", "face_id")}
    out["near_count"] = sum(v["near_count"] for v in views)
    return out


# ---- test meshes (generated, never committed) ------------------------------------------------------------------------------------
def cube(half=1.0):
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32) * np.float32(half)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    rng = np.random.default_rng(11)
    return {"vertices": v, "faces": f, "colors": rng.integers(0, 256, (8, 3)).astype(np.uint8)}


def icosphere(subdivisions, radius=1.0):
    """20 * 4^subdivisions triangles on a sphere (5 subdivisions: 20480), colours a smooth function of the direction."""
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    v = np.array(v)
    col = np.clip(127.5 + 127.5 * np.stack([v[:, 0], v[:, 1], np.sin(5 * v[:, 2])], axis=1), 0, 255).astype(np.uint8)
    return {"vertices": (v * radius).astype(np.float32), "faces": np.array(f, dtype=np.int32), "colors": col}
