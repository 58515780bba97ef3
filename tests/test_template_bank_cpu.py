"""CPU: the raster oracle (tests/render_oracle.py) against closed-form answers that do not come from it, and the host side of
picopose_amd/provider/template_bank.py — load_ply, the diameter / pose recipe, the fixture's provenance — plus the argument
checks of pp_render_views / pp_template_extents / pp_templates_crop through the ABI (no GPU)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_oracle as ro  # noqa: E402

from picopose_amd.provider import template_bank as tb  # noqa: E402

U = 2.0 ** -24                                               # float32 unit roundoff
K_EXACT = np.array([[512.0, 0, 320.0], [0, 512.0, 240.0], [0, 0, 1.0]])      # with z0 = 2: u = 256 X + 320, exact for dyadic X
Z0 = 2.0


def _pose(R=np.eye(3), t=(0, 0, Z0)):
    P = np.eye(4, dtype=np.float32)
    P[:3, :3], P[:3, 3] = R, t
    return P


def _screen_quad(u0, u1, v0, v1):
    """Object-frame corners (z = 0) that project exactly onto (u, v) under K_EXACT at depth Z0: order TL, TR, BL, BR."""
    return np.array([[(u - 320) / 256, (v - 240) / 256, 0.0] for v in (v0, v1) for u in (u0, u1)], dtype=np.float32)


@pytest.mark.parametrize("box", [(256.0, 384.0, 208.0, 272.0), (100.5, 200.25, 31.75, 90.0)])
def test_oracle_fronto_parallel_square(box):
    """(a) Edges on sample centres and between them.  Covered: u0 <= x < u1 and v0 <= y < v1 (left and top edges own their samples,
    right and bottom ones do not).  Depth: the weights sum to 1 exactly in real arithmetic and 1 / Zc = 0.5 exactly, so Z differs from
    z0 only by the roundings of item 6: two conversions, a division and a product per weight, two sums, one reciprocal — at most
    7 roundings on any path, |Z - z0| <= 8 u z0.  depth_mm = 2000 exactly.  Colour: the corners carry an affine ramp, which the
    barycentric blend reproduces; the same 8 u relative error on values <= 255 plus the rounding to uint8."""
    u0, u1, v0, v1 = box
    v = _screen_quad(u0, u1, v0, v1)
    f = np.array([[0, 1, 3], [0, 3, 2]], dtype=np.int32)
    col = np.array([[10, 0, 255], [210, 0, 255], [50, 0, 255], [250, 0, 255]], dtype=np.uint8)       # 10 + 200 s + 40 t
    r = ro.render_view(v, f, col, _pose(), K_EXACT, 480, 640)
    yy, xx = np.meshgrid(np.arange(480), np.arange(640), indexing="ij")
    want = (xx >= u0) & (xx < u1) & (yy >= v0) & (yy < v1)
    assert np.array_equal(r["face_id"] >= 0, want) and np.array_equal(r["rgba"][..., 3] == 255, want)
    assert np.all(r["rgba"][~want] == 0) and np.all(r["depth_mm"][~want] == 0)
    assert np.abs(r["depth_m"][want].astype(np.float64) - Z0).max() <= 8 * U * Z0
    assert np.all(r["depth_mm"][want] == 2000)
    ramp = 10 + 200 * (xx - u0) / (u1 - u0) + 40 * (yy - v0) / (v1 - v0)
    assert np.abs(r["rgba"][..., 0].astype(np.float64) - ramp)[want].max() <= 0.5 + 255 * 8 * U
    assert np.all(r["rgba"][want][:, 1] == 0) and np.all(r["rgba"][want][:, 2] == 255)
    assert r["near_count"] == 0


def test_oracle_tessellated_quad_covers_every_sample_once():
    """(b) 12 x 12 cells, 288 triangles with random diagonals and windings, interior vertices jittered by up to 1.5 px (cells of
    6.75 px cannot fold), the border on exact 1/256 px positions: without a depth test every sample with u0 <= x < u1, v0 <= y < v1
    is covered exactly once and no other sample at all."""
    rng = np.random.default_rng(7)
    n, u0, v0, step = 12, 100.25, 50.5, 6.75
    g = np.stack(np.meshgrid(u0 + step * np.arange(n + 1), v0 + step * np.arange(n + 1), indexing="xy"), axis=-1)
    g[1:-1, 1:-1] += rng.uniform(-1.5, 1.5, (n - 1, n - 1, 2))
    v = np.concatenate([(g[..., :1] - 320) / 256, (g[..., 1:] - 240) / 256, np.zeros((n + 1, n + 1, 1))], axis=-1).reshape(-1, 3)
    faces = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            tris = [[a, b, d], [a, d, c]] if rng.random() < 0.5 else [[a, b, c], [b, d, c]]
            faces += [t if rng.random() < 0.5 else t[::-1] for t in tris]
    cnt = ro.coverage_counts(v.astype(np.float32), np.array(faces, dtype=np.int32), _pose(), K_EXACT, 240, 320)
    yy, xx = np.meshgrid(np.arange(240), np.arange(320), indexing="ij")
    inside = (xx >= u0) & (xx < u0 + n * step) & (yy >= v0) & (yy < v0 + n * step)
    assert len(faces) == 288 and np.array_equal(cnt, inside.astype(np.int64))
    # a zero-area triangle covers nothing, wherever it lies
    z = ro.coverage_counts(v.astype(np.float32), np.array([[0, 6, 12], [5, 5, 70]], dtype=np.int32), _pose(), K_EXACT, 240, 320)
    assert z.sum() == 0


def test_oracle_tilted_plane_depth():
    """(c) A quad in the plane z_obj = 0 rotated 35 deg about y and 20 deg about x, wholly inside the frame.  With n = R e_z the
    plane's inverse depth is affine in the sample: 1 / Z = n . d / n . t, d = ((x - cx) / fx, (y - cy) / fy, 1).  The rendered
    1 / Z is affine between the SNAPPED vertex positions with the vertices' own 1 / Zc, so it is the analytic plane shifted in screen
    by at most the snap error per axis, e = 1/512 px + the float32 error of u (three roundings of a value below W: 3 u W), i.e.
    |d(1/Z)| <= g e with g = (|n_x| / fx + |n_y| / fy) / |n . t|; the vertices' Zc carry 3 roundings (relative 3 u) and item 6 adds
    at most 8: |Z - Z_analytic| <= Z^2 g e + 11 u Z."""
    ax, ay = np.deg2rad(20), np.deg2rad(35)
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    P = _pose(Rx @ Ry, (0.02, -0.01, 1.5))
    v = np.array([[-0.4, -0.3, 0], [0.4, -0.3, 0], [-0.4, 0.3, 0], [0.4, 0.3, 0]], dtype=np.float32)
    K = tb.TEMPLATE_K
    r = ro.render_view(v, np.array([[0, 1, 3], [0, 3, 2]], dtype=np.int32), np.zeros((4, 3), np.uint8), P, K, 480, 640)
    hit = r["face_id"] >= 0
    assert 20000 < hit.sum() < 480 * 640 and not hit[0].any() and not hit[:, 0].any() and not hit[-1].any() and not hit[:, -1].any()
    Pd = P.astype(np.float64)
    n, t = Pd[:3, 2], Pd[:3, 3]
    yy, xx = np.meshgrid(np.arange(480.0), np.arange(640.0), indexing="ij")
    d = np.stack([(xx - K[0, 2]) / K[0, 0], (yy - K[1, 2]) / K[1, 1], np.ones_like(xx)], axis=-1)
    Za = (n @ t) / (d @ n)
    g = (abs(n[0]) / K[0, 0] + abs(n[1]) / K[1, 1]) / abs(n @ t)
    e = 1 / 512 + 3 * U * 640
    bound = Za ** 2 * g * e + 11 * U * Za
    err = np.abs(r["depth_m"].astype(np.float64) - Za)
    print("tilted plane: max |Z - Za| / bound =", (err / bound)[hit].max())
    assert np.all(err[hit] <= bound[hit])


def test_oracle_icosphere_depth_between_sphere_and_sag():
    """(d) Icosphere of radius r (5120 triangles) at the reference's distance (t = (0, 0, diameter)), three reference views.  The
    mesh is inscribed in the sphere, so along a sample's ray the surface is never in front of the sphere: Z >= Z_sphere.  Behind it,
    the surface point X = Z d lies no deeper inside the sphere than the mesh's sag: r - |X - c| <= sag = r - min over faces of the
    distance from the centre (the face centroid's norm and, to be exact for faces that are not equilateral, the face plane's
    distance, computed here).  (Measured along the ray the gap grows without bound towards the silhouette, so the sag is
    compared radially, as the bank test does.)  Both sides allow the snap shift of c) moved to the surface, e Z / f sideways — a
    radial change of at most that — plus 11 u Z."""
    r0 = 0.05
    m = ro.icosphere(4, r0)
    v, f = m["vertices"].astype(np.float64), m["faces"]
    tri = v[f]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    plane = np.abs(np.einsum("ij,ij->i", nrm / np.linalg.norm(nrm, axis=1, keepdims=True), tri[:, 0]))
    sag = r0 - min(np.linalg.norm(tri.mean(axis=1), axis=1).min(), plane.min())
    assert 0 < sag < 0.01 * r0
    K = tb.TEMPLATE_K
    views = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "template_view_poses_level1.npy"))[[0, 57, 161]]
    poses = tb.template_object_poses(views, m["vertices"]).astype(np.float32)
    assert np.allclose(poses[:, 2, 3], r0 * 4 * 3 ** 0.5)
    yy, xx = np.meshgrid(np.arange(480.0), np.arange(640.0), indexing="ij")
    d = np.stack([(xx - K[0, 2]) / K[0, 0], (yy - K[1, 2]) / K[1, 1], np.ones_like(xx)], axis=-1)
    for P in poses:
        r = ro.render_view(m["vertices"], f, m["colors"], P, K, 480, 640)
        hit = r["face_id"] >= 0
        c = P[:3, 3].astype(np.float64)
        dd, dc = (d * d).sum(-1), d @ c
        disc = dc ** 2 - dd * (c @ c - r0 ** 2)
        assert hit.sum() > 15000 and np.all(disc[hit] > 0)        # every covered ray meets the sphere
        Zs = (dc - np.sqrt(np.where(disc > 0, disc, 0))) / dd
        Z = r["depth_m"].astype(np.float64)
        tol = (1 / 512 + 3 * U * 640) * Z / min(K[0, 0], K[1, 1]) + 11 * U * Z
        rad = np.linalg.norm(Z[..., None] * d - c, axis=-1)
        slope = np.sqrt(dd) * r0 / np.sqrt(np.where(disc > 0, disc, 1))      # dZ per unit of radial change at the sphere
        assert np.all((Z >= Zs - tol * np.maximum(slope, 1))[hit])
        assert np.all((rad <= r0 + tol)[hit]) and np.all((rad >= r0 - sag - tol)[hit])


# ---- host code ----------------------------------------------------------------------------------------------------------------
def _write_ply(path, v, f, colors=None, normals=False, binary=False, index_name="vertex_indices", alpha=False, extra_header=()):
    props = [("x", "f4"), ("y", "f4"), ("z", "f4")]
    if normals:
        props += [("nx", "f4"), ("ny", "f4"), ("nz", "f4")]
    if colors is not None:
        props += [("red", "u1"), ("green", "u1"), ("blue", "u1")] + ([("alpha", "u1")] if alpha else [])
    names = {"f4": "float", "u1": "uchar"}
    head = ["ply", "format " + ("binary_little_endian" if binary else "ascii") + " 1.0", "comment generated by the test",
            *extra_header, f"element vertex {len(v)}"]
    head += [f"property {names[t]} {n}" for n, t in props]
    head += [f"element face {len(f)}", f"property list uchar int {index_name}", "end_header"]
    tab = np.zeros(len(v), dtype=[(n, "<" + t) for n, t in props])
    tab["x"], tab["y"], tab["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals:
        tab["nx"], tab["ny"], tab["nz"] = 0.0, 0.0, 1.0
    if colors is not None:
        tab["red"], tab["green"], tab["blue"] = colors[:, 0], colors[:, 1], colors[:, 2]
        if alpha:
            tab["alpha"] = 255
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            fh.write(tab.tobytes())
            ft = np.zeros(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
            ft["n"], ft["i"] = 3, f
            fh.write(ft.tobytes())
        else:
            for row in tab:
                fh.write((" ".join(repr(float(x)) if isinstance(x, np.floating) else str(int(x)) for x in row) + "\n").encode("ascii"))
            for tri in f:
                fh.write(("3 " + " ".join(str(int(i)) for i in tri) + "\n").encode("ascii"))


@pytest.mark.parametrize("binary", [False, True])
def test_load_ply_round_trips_bit_for_bit(tmp_path, binary):
    m = ro.icosphere(1, 37.5)
    v, f, c = m["vertices"] + np.float32(0.1), m["faces"], m["colors"]
    for k, kw in enumerate(({}, {"colors": c}, {"colors": c, "normals": True}, {"colors": c, "alpha": True, "index_name": "vertex_index"},
                            {"normals": True, "index_name": "vertex_index"})):
        p = str(tmp_path / f"m{k}.ply")
        _write_ply(p, v, f, binary=binary, **kw)
        got = tb.load_ply(p)
        assert got["vertices"].dtype == np.float32 and got["faces"].dtype == np.int32
        assert np.array_equal(got["vertices"], v) and np.array_equal(got["faces"], f)
        if "colors" in kw:
            assert got["colors"].dtype == np.uint8 and np.array_equal(got["colors"], c)
        else:
            assert got["colors"] is None


def test_load_ply_malformed_cases_raise(tmp_path):
    m = ro.cube(10.0)
    v, f = m["vertices"], m["faces"]
    good = str(tmp_path / "good.ply")
    _write_ply(good, v, f, binary=True)
    raw = open(good, "rb").read()

    def variant(name, data):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        return p

    with pytest.raises(ValueError, match="big-endian"):
        tb.load_ply(variant("be.ply", raw.replace(b"binary_little_endian", b"binary_big_endian")))
    with pytest.raises(ValueError, match="not a PLY"):
        tb.load_ply(variant("magic.ply", b"obj" + raw[3:]))
    with pytest.raises(ValueError, match="'face'"):
        tb.load_ply(variant("noface.ply", raw.replace(b"element face 12\nproperty list uchar int vertex_indices\n", b"")))
    with pytest.raises(ValueError, match="'vertex'"):
        tb.load_ply(variant("novertex.ply", b"ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n"))
    with pytest.raises(ValueError, match="'z'"):
        tb.load_ply(variant("noz.ply", raw.replace(b"property float z\n", b"")))
    with pytest.raises(ValueError, match="truncated"):
        tb.load_ply(variant("short.ply", raw[:-5]))
    quad = str(tmp_path / "quad.ply")
    open(quad, "wb").write(b"ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
                           b"property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    with pytest.raises(ValueError, match="triangle"):
        tb.load_ply(quad)
    binq = raw[:raw.find(b"end_header") + 11] + raw[raw.find(b"end_header") + 11:][:8 * 12] + b"\x04" + raw[-13 * 12 + 1:]
    with pytest.raises(ValueError, match="not a triangle"):
        tb.load_ply(variant("binquad.ply", binq))


def test_diameter_and_object_poses_equal_the_reference_expressions(golden_dir):
    rng = np.random.default_rng(3)
    v = (rng.normal(size=(500, 3)) * [30, 80, 55] + [5, -7, 11]).astype(np.float32)
    extents = (v.astype(np.float64).max(axis=0) - v.astype(np.float64).min(axis=0)) * 2      # trimesh.py:20-23 (mesh.extents * 2)
    assert tb.mesh_diameter(v) == np.linalg.norm(extents)
    views = np.load(os.path.join(golden_dir, "template_view_poses_level1.npy"))
    want = views.copy()                                                                         # render_bop_templates.py:109-111
    want[:, :3, 3] = np.array([0, 0, np.linalg.norm(extents)])[None].repeat(len(views), axis=0)
    got = tb.template_object_poses(views, v)
    assert got.dtype == np.float64 and np.array_equal(got, want) and not np.array_equal(views, want)
    assert np.array_equal(tb.TEMPLATE_K, np.array([572.4114, 0.0, 320, 0.0, 573.57043, 240, 0.0, 0.0, 1.0]).reshape(3, 3))


def test_view_pose_fixture_is_the_reference_file(golden_dir):
    ref = os.path.join(os.environ.get("PICOPOSE_REFERENCE", "/root/reference"), "rendering/src/lib3d/predefined_poses/obj_poses_level1.npy")
    ours = os.path.join(golden_dir, "template_view_poses_level1.npy")
    a = np.load(ours)
    assert a.shape == (162, 4, 4) and np.allclose(np.einsum("vij,vkj->vik", a[:, :3, :3], a[:, :3, :3]), np.eye(3), atol=1e-9)
    if not os.path.exists(ref):
        pytest.skip("the reference tree is only present in the build container")
    assert open(ours, "rb").read() == open(ref, "rb").read()


def test_mesh_validation_raises_value_errors():
    m = ro.cube(10.0)
    bad = dict(m, faces=m["faces"].copy())
    bad["faces"][7, 1] = 8
    with pytest.raises(ValueError, match="face 7"):
        tb._mesh_arrays(bad)
    bad["faces"][7, 1] = -1
    with pytest.raises(ValueError, match="face 7"):
        tb._mesh_arrays(bad)
    with pytest.raises(ValueError, match="integer"):
        tb._mesh_arrays(dict(m, faces=m["faces"].astype(np.float32)))
    with pytest.raises(ValueError, match="non-finite"):
        tb._mesh_arrays(dict(m, vertices=m["vertices"] * np.float32(np.inf)))
    with pytest.raises(ValueError, match="colors"):
        tb._mesh_arrays(dict(m, colors=m["colors"].astype(np.float32)))
    v, f, c = tb._mesh_arrays(dict(m, colors=None, faces=m["faces"].astype(np.int64)[:, ::-1]))
    assert f.dtype == np.int32 and f.flags.c_contiguous and np.all(c == 128)
    with pytest.raises(ValueError, match="units"):
        tb._unit_scale("cm", m["vertices"])
    assert tb._unit_scale("auto", m["vertices"]) == 1e-3 and tb._unit_scale("auto", m["vertices"] / 1000) == 1.0


def test_render_abi_argument_validation_needs_no_gpu():
    from picopose_amd import _lib

    L = _lib.lib()
    assert {"pp_render_views", "pp_render_workspace_bytes", "pp_template_extents", "pp_templates_crop"} <= set(_lib.declared_symbols())
    buf = (ctypes.c_char * 1024)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    need = ctypes.c_size_t()
    assert L.pp_render_workspace_bytes(480, 640, 20480, 162, ctypes.byref(need)) == 0
    assert need.value == 256 + 162 * (480 * 640 + 20480) * 8
    for args in ((0, 640, 12, 1), (480, 0, 12, 1), (480, 640, 0, 1), (480, 640, 12, 0), (50000, 50000, 12, 1)):
        assert L.pp_render_workspace_bytes(*args, ctypes.byref(need)) == -1, args
    assert L.pp_render_workspace_bytes(480, 640, 12, 1, None) == -1
    i32 = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    one = 256 + (480 * 640 + 2) * 8

    def render(verts=p, nv=4, faces=p, faces_h=i32(0, 1, 2, 0, 2, 3), nf=2, colors=p, poses=p, V=3, fx=500.0, fy=500.0, H=480, W=640,
               near=1e-3, ws=p, ws_bytes=one, rgba=p, dmm=p, cnt=p):
        return L.pp_render_views(verts, nv, faces, faces_h, nf, colors, poses, V, fx, fy, 320.0, 240.0, H, W, near, ws, ws_bytes, rgba,
                                 dmm, None, None, cnt, None)

    for kw in ({"verts": None}, {"faces": None}, {"faces_h": None}, {"colors": None}, {"poses": None}, {"ws": None}, {"rgba": None},
               {"dmm": None}, {"cnt": None}, {"nv": 0}, {"nf": 0}, {"V": 0}, {"V": -2}, {"H": 0}, {"W": 0}, {"H": 50000, "W": 50000},
               {"near": 0.0}, {"near": -1.0}, {"fx": 0.0}, {"fy": 0.0},
               {"faces_h": i32(0, 1, 2, 0, 2, 4)}, {"faces_h": i32(0, -1, 2, 0, 2, 3)}):       # an index outside [0, Nv)
        assert render(**kw) == -1, kw
    assert render(ws_bytes=one - 1) == -2 and render(ws_bytes=0) == -2 and render(ws=p + 64) == -2      # PP_EWORKSPACE

    assert L.pp_template_extents(None, 3, 480, 640, p, None, None) == -1 and L.pp_template_extents(p, 3, 480, 640, None, None, None) == -1
    for V, H, W in ((0, 480, 640), (3, 0, 640), (3, 480, 0), (3, 50000, 50000)):
        assert L.pp_template_extents(p, V, H, W, p, None, None) == -1
    mean, std = (ctypes.c_double * 3)(0.5, 0.5, 0.5), (ctypes.c_double * 3)(0.2, 0.2, 0.2)

    def crop(rgba=p, depth=p, V=2, H=480, W=640, boxes=p, boxes_h=i32(0, 100, 0, 100, 380, 480, 540, 640), fx=500.0, S=224, P=64, mean3=mean,
             std3=std, rgb=p, mask=p, pts=p):
        return L.pp_templates_crop(rgba, depth, 0, V, H, W, boxes, boxes_h, fx, 500.0, 320.0, 240.0, S, P, 0, mean3, std3, rgb, mask, pts, None)

    for kw in ({"rgba": None}, {"depth": None}, {"boxes": None}, {"boxes_h": None}, {"mean3": None}, {"std3": None}, {"rgb": None},
               {"mask": None}, {"pts": None}, {"V": 0}, {"V": 70000}, {"H": 0}, {"W": 0}, {"S": 0}, {"P": 0}, {"S": 5000}, {"fx": 0.0},
               {"boxes_h": i32(0, 100, 0, 100, 380, 481, 540, 640)}, {"boxes_h": i32(0, 100, 0, 100, 380, 480, 540, 641)},
               {"boxes_h": i32(-1, 100, 0, 100, 380, 480, 540, 640)}, {"boxes_h": i32(50, 50, 0, 100, 380, 480, 540, 640)},
               {"boxes_h": i32(0, 100, 30, 20, 380, 480, 540, 640)}):
        assert crop(**kw) == -1, kw
