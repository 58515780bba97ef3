"""Numpy statement of the shading contract of include/picopose_hip.h ("THE SHADING CONTRACT", S2-S8), written from that text and
built on render_oracle / texture_oracle for everything the raster and texture contracts already fix: coverage, depth, the
perspective weights and the base colour (the unlit pixel).  Every float operation is one float32 numpy operation in the stated
order; sqrt and / are correctly rounded in numpy as in the kernels.  It is checked against float64 closed-form answers in
tests/test_shaded_bank_cpu.py; the GPU kernels are held to it bit for bit in tests/test_shaded_bank_gpu.py."""
import numpy as np

import render_oracle as ro
import texture_oracle as to
from render_oracle import F


def vertex_face_csr(faces, n_vertices):
    """S8's adjacency, written independently of the package's: for every vertex the faces that name it, ascending, once per corner."""
    lists = [[] for _ in range(n_vertices)]
    for fi, tri in enumerate(np.asarray(faces).tolist()):
        for v in tri:
            lists[v].append(fi)
    offsets = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    return offsets, np.array([fi for l in lists for fi in l], dtype=np.int32)


def _cross(e1, e2):
    """(a b) - (c d) per component, float32; e1, e2 lists of three arrays."""
    return [(e1[1] * e2[2]) - (e1[2] * e2[1]), (e1[2] * e2[0]) - (e1[0] * e2[2]), (e1[0] * e2[1]) - (e1[1] * e2[0])]


def _normalise(n):
    """S3's len2 and division -> unit components (garbage where ok is false), ok = len2 > 0."""
    len2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    ok = len2 > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt(np.where(ok, len2, F(1)))
        return [c / ln for c in n], ok


def vertex_normals(vertices, faces):
    """S8 -> (Nv, 3) float32."""
    v, f = np.asarray(vertices, dtype=F), np.asarray(faces, dtype=np.int64)
    off, adj = vertex_face_csr(f, len(v))
    e1 = [v[f[:, 1], c] - v[f[:, 0], c] for c in range(3)]
    e2 = [v[f[:, 2], c] - v[f[:, 0], c] for c in range(3)]
    with np.errstate(over="ignore", invalid="ignore"):
        fn = np.stack(_cross(e1, e2), axis=1)                    # (Nf, 3)
        acc = np.zeros((len(v), 3), dtype=F)
        deg = np.diff(off)
        for j in range(int(deg.max()) if len(deg) else 0):       # the j-th incident face of every vertex that has one: sequential adds
            has = np.where(deg > j)[0]
            acc[has] = acc[has] + fn[adj[off[has] + j]]
        n, ok = _normalise([acc[:, 0], acc[:, 1], acc[:, 2]])
    return np.where(ok[:, None], np.stack(n, axis=1), F(0)).astype(F)


def shade(tri, pose, vertices, face, p, q, base, lights4, ambient, normals=None, tone=None):
    """S2-S6 for covered samples: face (n,) the winning faces, p, q item 6's weights, base (n, 3) uint8 -> (out (n, 3) uint8, s (n,) f32)."""
    P, v = np.asarray(pose, dtype=F), np.asarray(vertices, dtype=F)
    ids = tri.ids[face]                                          # (n, 3): the corners in the order item 4 left them
    C = []
    for k in range(3):
        X, Y, Z = v[ids[:, k], 0], v[ids[:, k], 1], v[ids[:, k], 2]
        C.append([((P[r, 0] * X + P[r, 1] * Y) + P[r, 2] * Z) + P[r, 3] for r in range(3)])
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        pos = [((p[0] * C[0][c] + p[1] * C[1][c]) + p[2] * C[2][c]) / q for c in range(3)]          # S2
        if normals is None:                                                                         # S3
            n = _cross([C[1][c] - C[0][c] for c in range(3)], [C[2][c] - C[0][c] for c in range(3)])
        else:
            N = np.asarray(normals, dtype=F)
            o = [(p[0] * N[ids[:, 0], c] + p[1] * N[ids[:, 1], c]) + p[2] * N[ids[:, 2], c] for c in range(3)]
            n = [(P[r, 0] * o[0] + P[r, 1] * o[1]) + P[r, 2] * o[2] for r in range(3)]
        n, ok = _normalise(n)
        flip = ((n[0] * pos[0] + n[1] * pos[1]) + n[2] * pos[2]) > 0
        n = [np.where(flip, -c, c) for c in n]
        s = np.zeros(len(face), dtype=F)
        for L in np.asarray(lights4, dtype=F).reshape(-1, 4):                                       # S4
            l = [L[c] - pos[c] for c in range(3)]
            d2 = (l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]
            ndl = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2]
            add = ok & (ndl > 0) & (d2 > 0)
            s = np.where(add, s + (L[3] * ndl) / (d2 * np.sqrt(d2)), s)
        m = F(ambient) + s                                                                          # S5
        val = np.asarray(base).astype(F) * m[:, None]
        if tone is None:                                                                            # S6
            out = np.fmin(np.fmax(np.floor(val + F(0.5)), F(0)), F(255)).astype(np.uint8)
        else:
            T = len(tone)
            idx = np.rint(np.fmin(val / F(255), F(1)) * F(T - 1)).astype(np.int64)
            out = np.asarray(tone, dtype=np.uint8)[np.clip(idx, 0, T - 1)]
    return out, s


def render_view(mesh, pose, K, H, W, lights4, ambient, normals=None, base_color=None, tone=None, near=1e-3):
    """One lit view of `mesh` ({"vertices", "faces"} with "colors", or "texture" + "face_uv", or neither when base_color is given).
    normals: None = flat, else (Nv, 3) object-space vertex normals.  -> rgba, depth_mm, depth_m, face_id as the unlit oracles give
    them (S7), "s" (H, W) float32 (the diffuse sum, 0 on background), near_count."""
    v, f = mesh["vertices"], mesh["faces"]
    if mesh.get("texture") is not None:
        out = to.render_view(v, f, mesh["face_uv"], mesh["texture"], pose, K, H, W, near)
    else:
        col = mesh.get("colors")
        out = ro.render_view(v, f, np.zeros((len(v), 3), np.uint8) if col is None else col, pose, K, H, W, near)
    assert base_color is not None or mesh.get("texture") is not None or mesh.get("colors") is not None
    rgba = out["rgba"].reshape(-1, 4).copy()
    smap = np.zeros(H * W, dtype=F)
    hit = np.where(out["face_id"].reshape(-1) >= 0)[0]
    if len(hit):
        tri = ro.Triangles(v, f, pose, ro._k4(K), H, W, near)
        face = out["face_id"].reshape(-1)[hit].astype(np.int64)
        w, inside = tri.weights(face, hit % W, hit // W)
        assert inside.all()
        p, q = tri.depth_terms(face, w)
        base = rgba[hit, :3] if base_color is None else np.tile(np.asarray(base_color, dtype=np.uint8), (len(hit), 1))
        rgba[hit, :3], smap[hit] = shade(tri, pose, v, face, p, q, base, lights4, ambient, normals, tone)
    return {"rgba": rgba.reshape(H, W, 4), "depth_mm": out["depth_mm"], "depth_m": out["depth_m"], "face_id": out["face_id"],
            "s": smap.reshape(H, W), "near_count": out["near_count"]}


def render(mesh, poses, K, H, W, lights4, ambient, normals=None, base_color=None, tone=None, near=1e-3):
    """All views stacked; near_count summed."""
    views = [render_view(mesh, p, K, H, W, lights4, ambient, normals, base_color, tone, near) for p in poses]
    out = {k: np.stack([x[k] for x in views]) for k in ("rgba", "depth_mm", "depth_m", "face_id", "s")}
    out["near_count"] = sum(x["near_count"] for x in views)
    return out
