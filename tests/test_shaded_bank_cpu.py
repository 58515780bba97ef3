"""CPU: the shading oracle (tests/shading_oracle.py) against float64 answers that do not come from it, so that the GPU tests of
tests/test_shaded_bank_gpu.py inherit a trusted yardstick; the host side of shaded onboarding in
picopose_amd/provider/template_bank.py (template_lights, srgb_tone_table, load_ply's normals, the validation of `shading`); and
the argument checks of pp_vertex_normals / pp_render_views_lit through the ABI (no GPU)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_oracle as ro  # noqa: E402
import shading_oracle as so  # noqa: E402

from picopose_amd.provider import template_bank as tb  # noqa: E402

H, W = 48, 64
FOC, CX, CY = 32.0, 32.0, 24.0                                  # a wide camera: the frame spans +-45 degrees, so the fall-off shows
K_WIDE = np.array([[FOC, 0, CX], [0, FOC, CY], [0, 0, 1.0]])
BASE = np.array([200, 100, 50], dtype=np.uint8)


def _quad(half=8.0, reverse=False):
    """A square in the plane z = 0 of the object frame, larger than the frame once posed: two triangles."""
    v = np.array([[-half, -half, 0], [half, -half, 0], [-half, half, 0], [half, half, 0]], dtype=np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2]], dtype=np.int32)
    return {"vertices": v, "faces": f[:, [0, 2, 1]] if reverse else f}


def _pose(R=np.eye(3), t=(0, 0, 2.0)):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return P.astype(np.float32)


def _rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def _expected(pose, lights4, ambient, base=BASE, tone=None):
    """The float64 answer for the posed plane z_obj = 0, by ray casting: per pixel the hit point, the camera-facing unit normal, the
    Lambert sum -> (multiplier (H, W), colour (H, W, 3) float64 before rounding, the value S6 rounds)."""
    P = np.asarray(pose, dtype=np.float64)
    n, p0 = P[:3, 2], P[:3, 3]                                   # the plane's normal (the rotated object z axis) and a point of it
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.stack([(xs - CX) / FOC, (ys - CY) / FOC, np.ones_like(xs, dtype=np.float64)], axis=-1)
    t = (n @ p0) / (d @ n)
    pos = d * t[..., None]
    n = np.where((pos @ n)[..., None] > 0, -n, n)                # towards the camera
    s = np.zeros((H, W))
    for lx, ly, lz, inten in np.asarray(lights4, dtype=np.float64).reshape(-1, 4):
        l = np.array([lx, ly, lz]) - pos
        d2 = (l ** 2).sum(-1)
        ndl = (n * l).sum(-1)
        s += np.where(ndl > 0, inten * ndl / d2 ** 1.5, 0.0)
    m = ambient + s
    return m, base.astype(np.float64) * m[..., None]


def _round(val, tone=None):
    if tone is None:
        return np.minimum(np.floor(val + 0.5), 255)
    return tone[np.rint(np.minimum(val / 255.0, 1.0) * (len(tone) - 1)).astype(int)].astype(np.float64)


def _lit(mesh, pose, lights4, ambient, **kw):
    return so.render_view(mesh, pose, K_WIDE, H, W, np.asarray(lights4, dtype=np.float32), ambient, base_color=BASE, **kw)


def _assert_within_one_lsb(got, val, cover, tone=None):
    want = _round(val, tone)
    # a value within float32 noise of a rounding boundary may fall on either side of it: 1 LSB, as the issue allows
    assert np.abs(got["rgba"][..., :3].astype(np.float64) - want)[cover].max() <= 1
    assert (got["rgba"][..., :3].astype(np.float64) == want)[cover].mean() > 0.97          # and nearly every sample exactly


# ---- 1. the oracle against float64 ---------------------------------------------------------------------------------------------------
def test_facing_quad_under_a_headlight_has_the_inverse_square_centre_and_cubic_falloff():
    z, inten = 2.0, 4.8                                          # centre multiplier I / z^2 = 1.2: the brightest channel saturates
    got = _lit(_quad(), _pose(t=(0, 0, z)), [[0, 0, 0, inten]], 0.0)
    cover = got["face_id"] >= 0
    assert cover.all()
    m, val = _expected(_pose(t=(0, 0, z)), [[0, 0, 0, inten]], 0.0)
    ys, xs = np.mgrid[0:H, 0:W]
    r = np.sqrt(((xs - CX) * z / FOC) ** 2 + ((ys - CY) * z / FOC) ** 2 + z * z)
    assert np.allclose(m, inten / z ** 2 * (z / r) ** 3, rtol=1e-12)                       # the closed form the ray cast must equal
    assert abs(m[int(CY), int(CX)] - inten / z ** 2) < 1e-12 and m.min() < 0.45 * m.max()
    assert np.abs(got["s"].astype(np.float64) - m)[cover].max() < 1e-5
    _assert_within_one_lsb(got, val, cover)
    assert got["rgba"][int(CY), int(CX)].tolist() == [240, 120, 60, 255] and (got["rgba"][..., 0] == 240).sum() < 10
    bright = _lit(_quad(), _pose(t=(0, 0, z)), [[0, 0, 0, 2 * inten]], 0.0)
    assert bright["rgba"][int(CY), int(CX)].tolist() == [255, 240, 120, 255]               # saturation at 255
    tone = tb.srgb_tone_table(4096)
    _assert_within_one_lsb(_lit(_quad(), _pose(t=(0, 0, z)), [[0, 0, 0, inten]], 0.0, tone=tone), val, cover, tone)


@pytest.mark.parametrize("deg", [35.0, -60.0])
def test_tilted_quad_matches_the_ray_cast_plane(deg):
    pose = _pose(_rot_y(deg), (0.1, -0.2, 3.0))
    lights = [[0, 0, 0, 5.0], [0.5, -0.3, 0.0, 3.0], [-1.0, 1.0, -1.0, 6.0]]
    got = _lit(_quad(2.0), pose, lights, 0.05)
    cover = got["face_id"] >= 0
    assert cover.sum() > 400                                     # (a quad small enough to stay in front of the near plane)
    m, val = _expected(pose, lights, 0.05)
    assert m[cover].max() > 1.5 * m[cover].min()
    _assert_within_one_lsb(got, val, cover)
    # smooth normals that equal the face normal give the same multiplier (another arithmetic path: rotation of the object normal)
    smooth = _lit(_quad(2.0), pose, lights, 0.05, normals=np.tile(np.float32([0, 0, -1]), (4, 1)))
    _assert_within_one_lsb(smooth, val, cover)
    up = _lit(_quad(2.0), pose, lights, 0.05, normals=np.tile(np.float32([0, 0, 3.5]), (4, 1)))       # any length, either sign
    assert np.array_equal(up["rgba"], smooth["rgba"])


def test_a_light_behind_the_surface_contributes_nothing():
    pose = _pose(t=(0, 0, 2.0))
    front, behind = [0.3, 0.2, 0.5, 2.0], [0.0, 0.0, 3.0, 50.0]
    a = _lit(_quad(), pose, [front], 0.25)
    b = _lit(_quad(), pose, [behind, front], 0.25)
    assert np.array_equal(a["rgba"], b["rgba"]) and np.array_equal(a["s"], b["s"])
    only = _lit(_quad(), pose, [behind], 0.25)
    assert np.all(only["s"] == 0) and np.all(only["rgba"] == [50, 25, 13, 255])            # ambient alone: floor(0.25 base + 0.5)
    none = _lit(_quad(), pose, np.zeros((0, 4)), 0.25)
    assert np.array_equal(none["rgba"], only["rgba"])
    zero = _lit(_quad(), pose, [[0.3, 0.2, 0.5, 0.0]], 0.25)                                 # a light of intensity 0
    assert np.array_equal(zero["rgba"], only["rgba"])


def test_reversed_winding_gives_the_same_bytes():
    pose = _pose(_rot_y(40.0), (0.0, 0.1, 3.0))
    lights = [[0, 0, 0, 5.0], [0.5, -0.3, 0.0, 3.0]]
    a, b = _lit(_quad(2.0), pose, lights, 0.1), _lit(_quad(2.0, reverse=True), pose, lights, 0.1)
    for k in ("rgba", "depth_mm", "face_id", "s"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["face_id"] >= 0).sum() > 400 and len(np.unique(a["rgba"][..., 0])) > 20
    back = _lit(_quad(2.0), _pose(_rot_y(220.0), (0.0, 0.1, 3.0)), lights, 0.1)                 # seen from its back: still lit (two-sided)
    assert (back["face_id"] >= 0).sum() > 400 and (back["s"][back["face_id"] >= 0] > 0).all()


def test_identity_shading_returns_the_unlit_pixel():
    m = ro.icosphere(1, 0.5)
    pose = _pose(t=(0.1, 0.0, 2.0))
    unlit = ro.render_view(m["vertices"], m["faces"], m["colors"], pose, K_WIDE, H, W)
    lit = so.render_view(m, pose, K_WIDE, H, W, np.zeros((0, 4), np.float32), 1.0)
    assert np.array_equal(lit["rgba"], unlit["rgba"]) and (unlit["face_id"] >= 0).sum() > 40


# ---- 2. S8 -------------------------------------------------------------------------------------------------------------------------------
def _area_weighted_f64(v, f):
    v = v.astype(np.float64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, f[:, k], fn)
    return acc / np.linalg.norm(acc, axis=1, keepdims=True)


def test_vertex_normals_of_the_cube():
    """A corner's area-weighted normal is sign(v) (1, 1, 1) / sqrt(3) when the triangulation is the same on its three sides.  With
    two triangles per side that holds at the corners every side's diagonal meets (0 and 7 of render_oracle.cube); a corner that a
    diagonal misses gets one triangle from that side instead of two, and its exact normal is sign(v) (w_x, w_y, w_z) / |w| with
    w in {1, 2}.  All eight are checked against that exact answer, and a cube whose sides are split from their centres (the same at
    every corner) against (1, 1, 1) / sqrt(3) throughout."""
    m = ro.cube(0.4)
    n = so.vertex_normals(m["vertices"], m["faces"])
    assert n.dtype == np.float32 and n.shape == (8, 3)
    eps = np.finfo(np.float32).eps
    for c in (0, 7):
        assert np.abs(n[c] - np.sign(m["vertices"][c]) / np.sqrt(3)).max() <= 2 * eps
    count = np.zeros((8, 3))                                      # triangles per corner and axis-aligned side
    for tri in m["faces"]:
        axis = int(np.argmax(np.all(m["vertices"][tri] == m["vertices"][tri][0], axis=0)))
        count[tri, axis] += 1
    assert set(np.unique(count)) == {1.0, 2.0}
    want = np.sign(m["vertices"]) * count / np.linalg.norm(count, axis=1, keepdims=True)
    assert np.abs(n - want).max() <= 2 * eps
    v, f = list(m["vertices"]), []
    for (a, b, c), (a2, c2, d) in zip(m["faces"][0::2], m["faces"][1::2]):      # a side is (a, b, c) + (a, c, d): its ring is a b c d
        assert (a, c) == (a2, c2)
        v.append(np.mean([m["vertices"][i] for i in (a, b, c, d)], axis=0, dtype=np.float32))
        f += [[r0, r1, len(v) - 1] for r0, r1 in ((a, b), (b, c), (c, d), (d, a))]
    v = np.array(v, dtype=np.float32)
    f = np.array(f, dtype=np.int32)
    n = so.vertex_normals(v, f)
    assert np.abs(n[:8] - np.sign(v[:8]) / np.sqrt(3)).max() <= 2 * eps
    assert np.abs(n[8:] - v[8:] / np.float32(0.4)).max() <= 2 * eps                     # a side's centre: the side's normal


def test_vertex_normals_of_the_icosphere_and_degenerate_meshes():
    m = ro.icosphere(2, 0.5)
    n = so.vertex_normals(m["vertices"], m["faces"])
    unit = m["vertices"].astype(np.float64) / np.linalg.norm(m["vertices"].astype(np.float64), axis=1, keepdims=True)
    assert np.abs(n - _area_weighted_f64(m["vertices"], m["faces"])).max() < 1e-6
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
    # the area-weighted normal of this (not quite regular) inscribed mesh leaves the radial direction in proportion to the edge
    # length: 2.0e-2 at 2 subdivisions, half of it per further one (2.7e-3 at 5, 1.4e-3 at 6).  "Within 1e-3 of v / |v|" is therefore
    # a property of a sphere of 7 subdivisions or more, and is checked there (6.9e-4)
    assert 5e-3 < np.abs(n - unit).max() < 5e-2
    m = ro.icosphere(7, 0.5)
    n = so.vertex_normals(m["vertices"], m["faces"])
    unit = m["vertices"].astype(np.float64) / np.linalg.norm(m["vertices"].astype(np.float64), axis=1, keepdims=True)
    assert len(m["faces"]) == 327680 and np.abs(n - unit).max() < 1e-3
    # an unreferenced vertex and a vertex whose only face has no area: zeros; the others untouched
    c = ro.cube(0.4)
    v = np.concatenate([c["vertices"], np.float32([[9, 9, 9], [1, 2, 3]])])
    f = np.concatenate([c["faces"], np.int32([[0, 0, 9], [3, 9, 3]])])
    n2 = so.vertex_normals(v, f)
    assert np.all(n2[8:] == 0) and np.array_equal(n2[:8], so.vertex_normals(c["vertices"], c["faces"]))
    off, adj = tb.vertex_face_csr(f, len(v))
    off2, adj2 = so.vertex_face_csr(f, len(v))
    assert np.array_equal(off, off2) and np.array_equal(adj, adj2) and off.dtype == adj.dtype == np.int32
    assert off[8] == off[9] and off[10] - off[9] == 2                                    # vertex 8 unreferenced; vertex 9 named by two faces without area


# ---- 3. the host side --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe,count", [("blenderproc", 8), ("headlight", 1)])
@pytest.mark.parametrize("distance,key", [(0.35, 1.0), (1.7, 0.8)])
def test_template_lights_put_the_key_multiplier_on_a_facing_surface(recipe, count, distance, key):
    t = tb.template_lights(distance, recipe, key)
    L, inten = t["lights"], t["intensity"]
    assert L.shape == (count, 3) and inten.shape == (count,) and L.dtype == inten.dtype == np.float64
    assert np.all(inten == inten[0]) and inten[0] > 0
    to_light = L - np.array([0, 0, distance])
    ndl = to_light @ np.array([0.0, 0.0, -1.0])
    assert np.all(ndl > 0)
    s = (inten * ndl / np.linalg.norm(to_light, axis=1) ** 3).sum()
    assert abs(s - key) <= 1e-12
    if recipe == "blenderproc":                                   # blenderproc.py:29-33 in our frame: (x, -y, -z), z_blender in {0, 1}
        want = {(x, -y, -z) for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (0.0, 1.0)}
        assert {tuple(float(c) + 0.0 for c in row) for row in L} == {tuple(c + 0.0 for c in w) for w in want}
        assert np.all(L[:, 2] <= 0)                               # beside and behind the camera, never between it and the object
    else:
        assert np.all(L == 0) and abs(inten[0] - key * distance ** 2) <= 1e-12
    for bad in ({"distance_m": 0.0}, {"distance_m": float("nan")}, {"distance_m": 1.0, "recipe": "sun"}, {"distance_m": 1.0, "key": -1.0}):
        with pytest.raises(ValueError):
            tb.template_lights(**bad)


def test_srgb_tone_table_endpoints_and_monotonicity():
    for T in (2, 256, 4096, 65536):
        t = tb.srgb_tone_table(T)
        assert t.dtype == np.uint8 and t.shape == (T,) and t[0] == 0 and t[-1] == 255 and np.all(np.diff(t.astype(int)) >= 0)
    t = tb.srgb_tone_table()
    assert len(t) == 4096
    x = np.arange(4096) / 4095.0
    assert t[np.argmin(np.abs(x - 0.5))] in (187, 188) and t[np.argmin(np.abs(x - 0.2140))] in (127, 128)     # oetf(0.5) = 0.7354, oetf(0.214) = 0.5
    assert t[5] == round(12.92 * 5 / 4095 * 255)                  # the linear toe
    for T in (1, 0, 65537):
        with pytest.raises(ValueError):
            tb.srgb_tone_table(T)


def _write_ply(path, v, f, binary, normals=None, colors=None):
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals is not None else [])
    cols = [v] + ([normals] if normals is not None else [])
    with open(path, "wb") as fh:
        head = ["ply", "format " + ("binary_little_endian" if binary else "ascii") + " 1.0", f"element vertex {len(v)}"]
        head += [f"property float {n}" for n in props] + (["property uchar red", "property uchar green", "property uchar blue"] if colors is not None else [])
        head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        tab = np.concatenate(cols, axis=1).astype("<f4")
        for i in range(len(v)):
            if binary:
                fh.write(tab[i].tobytes() + (colors[i].tobytes() if colors is not None else b""))
            else:
                fh.write((" ".join([repr(float(x)) for x in tab[i]] + ([str(int(c)) for c in colors[i]] if colors is not None else [])) + "\n").encode("ascii"))
        for tri in f:
            fh.write(b"\x03" + np.asarray(tri, "<i4").tobytes() if binary else ("3 " + " ".join(str(int(i)) for i in tri) + "\n").encode("ascii"))


@pytest.mark.parametrize("binary", [False, True])
def test_load_ply_returns_the_normals_it_was_given(tmp_path, binary):
    m = ro.icosphere(1, 37.5)
    normals = np.random.default_rng(5).normal(size=(len(m["vertices"]), 3)).astype(np.float32)
    p = str(tmp_path / "m.ply")
    _write_ply(p, m["vertices"], m["faces"], binary, normals=normals, colors=m["colors"])
    got = tb.load_ply(p)
    assert got["normals"].dtype == np.float32 and got["normals"].flags.c_contiguous and np.array_equal(got["normals"], normals)
    assert np.array_equal(got["vertices"], m["vertices"]) and np.array_equal(got["faces"], m["faces"]) and np.array_equal(got["colors"], m["colors"])
    assert got["uv"] is None and got["face_uv"] is None and got["texture_file"] is None
    _write_ply(p, m["vertices"], m["faces"], binary)
    got = tb.load_ply(p)
    assert got["normals"] is None and got["colors"] is None and np.array_equal(got["vertices"], m["vertices"])
    assert set(got) == {"vertices", "faces", "colors", "uv", "face_uv", "normals", "texture_file"}


def test_malformed_shading_raises_before_any_device_work():
    m = ro.cube(0.4)
    poses = _pose()[None]
    ok = {"lights": np.zeros((2, 3)), "intensity": np.ones(2), "ambient": 0.1}
    bad = [{"lights": np.zeros((2, 2))}, {"lights": np.zeros(3)}, {"lights": np.zeros((17, 3)), "intensity": np.ones(17)},
           {"lights": np.full((2, 3), np.nan)}, {"lights": np.full((2, 3), 1e39)}, {"lights": "here"}, {"intensity": np.ones(3)},
           {"intensity": [1.0, -1.0]}, {"intensity": [1.0, np.inf]}, {"intensity": None}, {"ambient": -0.1}, {"ambient": float("nan")},
           {"ambient": float("inf")}, {"ambient": "dim"}, {"normals": "auto"}, {"normals": None}, {"base_color": (1, 2)},
           {"base_color": (1, 2, 256)}, {"base_color": (0.5, 0.5, 0.5)}, {"base_color": (-1, 0, 0)}, {"tone": "gamma"},
           {"tone": np.zeros(1, np.uint8)}, {"tone": np.zeros(65537, np.uint8)}, {"tone": np.zeros(16, np.float32)},
           {"tone": np.zeros((4, 4), np.uint8)}, {"colour": (1, 2, 3)}]
    for kw in bad:
        with pytest.raises(ValueError):
            tb.render_views(m, poses, units="m", device="no_such_device", shading=dict(ok, **kw))
    for shading in ("phong", 3, ["tless"]):
        with pytest.raises(ValueError):
            tb.render_views(m, poses, units="m", device="no_such_device", shading=shading)
    with pytest.raises(ValueError, match="normals must be"):
        tb.render_views(dict(m, normals=np.zeros((7, 3), np.float32)), poses, units="m", device="no_such_device", shading=dict(ok, normals="smooth"))
    with pytest.raises(ValueError):
        tb.render_templates(m, poses, units="m", device="no_such_device", shading={"ambient": -1.0})
    # what a well-formed description parses to
    lights4, ambient, smooth, base, tone = tb._parse_shading(tb.Shading(**ok, normals="smooth", base_color=[1, 2, 3], tone="srgb"), 1.0)
    assert lights4.shape == (2, 4) and lights4.dtype == np.float32 and ambient == 0.1 and smooth and base.tolist() == [1, 2, 3]
    assert np.array_equal(tone, tb.srgb_tone_table(4096))
    lights4, ambient, smooth, base, tone = tb._parse_shading("tless", 0.3)
    t = tb.template_lights(0.3)
    assert np.array_equal(lights4, np.concatenate([t["lights"], t["intensity"][:, None]], axis=1).astype(np.float32))
    assert (ambient, smooth, base.tolist(), tone) == (0.0, False, [102, 102, 102], None)
    assert tb._parse_shading({}, 1.0)[0].shape == (0, 4)


# ---- 4. the C ABI's argument checks (they run before any launch: no GPU) ----------------------------------------------------------------
def test_shading_abi_argument_validation_needs_no_gpu():
    from picopose_amd import _lib

    L = _lib.lib()
    assert {"pp_vertex_normals", "pp_render_views_lit"} <= set(_lib.declared_symbols())
    buf = (ctypes.c_char * 2048)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256

    def normals(verts=p, nv=8, faces=p, nf=12, off=p, adj=p, out=p):
        return L.pp_vertex_normals(verts, nv, faces, nf, off, adj, out, None)

    for kw in ({"verts": None}, {"faces": None}, {"off": None}, {"adj": None}, {"out": None}, {"nv": 0}, {"nf": 0}, {"nf": 2 ** 31 // 3 + 1},
               {"verts": p + 2}, {"faces": p + 1}, {"off": p + 2}, {"adj": p + 3}, {"out": p + 2}):
        assert normals(**kw) == -1, kw
    i32 = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    f32 = lambda *v: (ctypes.c_float * len(v))(*v)  # noqa: E731
    one = 256 + (480 * 640 + 2) * 8
    two_lights, grey = f32(0, 0, 0, 1, 1, 1, 0, 2), (ctypes.c_ubyte * 3)(102, 102, 102)
    many = f32(*([0.0] * 68))

    def lit(verts=p, nv=4, faces=p, faces_h=i32(0, 1, 2, 0, 2, 3), nf=2, colors=p, uv=None, mip=None, Wt=0, Ht=0, poses=p, V=3, fx=500.0,
            fy=500.0, H=480, W=640, near=1e-3, ws=p, ws_bytes=one, rgba=p, dmm=p, cnt=p, lights=two_lights, nl=2, ambient=0.1, mode=0,
            nrm=None, base=None, tone=None, T=0):
        return L.pp_render_views_lit(verts, nv, faces, faces_h, nf, colors, uv, mip, Wt, Ht, poses, V, fx, fy, 320.0, 240.0, H, W, near, ws,
                                     ws_bytes, rgba, dmm, None, None, cnt, lights, nl, ambient, mode, nrm, base, tone, T, None)

    tex = {"colors": None, "uv": p, "mip": p, "Wt": 16, "Ht": 8}
    for kw in ({"nl": -1}, {"nl": 17, "lights": many}, {"lights": None}, {"lights": f32(0, 0, float("nan"), 1), "nl": 1},
               {"lights": f32(0, 0, 0, float("inf")), "nl": 1}, {"lights": f32(0, 0, 0, -1), "nl": 1}, {"ambient": -0.5},
               {"ambient": float("nan")}, {"ambient": float("inf")}, {"mode": 1}, {"mode": 2}, {"mode": -1},        # smooth without normals
               {"colors": None}, dict(tex, colors=p),                                                              # no source / both
               dict(tex, mip=None), dict(tex, uv=None), dict(tex, Wt=0), dict(tex, Ht=16385), dict(tex, uv=p + 2), dict(tex, mip=p + 1),
               {"tone": p, "T": 1}, {"tone": p, "T": 0}, {"tone": p, "T": 65537}, {"tone": None, "T": 16},
               {"lights": ctypes.addressof(two_lights) + 2}, {"mode": 1, "nrm": p + 2},
               # what the existing entries reject
               {"verts": None}, {"faces": None}, {"faces_h": None}, {"poses": None}, {"ws": None}, {"rgba": None}, {"dmm": None}, {"cnt": None},
               {"nv": 0}, {"nf": 0}, {"V": 0}, {"H": 0}, {"W": 0}, {"H": 50000, "W": 50000}, {"near": 0.0}, {"fx": 0.0}, {"fy": 0.0},
               {"rgba": p + 2}, {"faces_h": i32(0, 1, 2, 0, 2, 4)}, {"faces_h": i32(0, -1, 2, 0, 2, 3)},
               dict(tex, verts=None), {"colors": None, "base": grey, "rgba": None}, {"mode": 1, "nrm": p, "V": 0},
               {"tone": p, "T": 4096, "H": 0}, {"nl": 0, "lights": None, "W": 0}):
        assert lit(**kw) == -1, kw
    # each well-formed description gets past the shading checks: it is the workspace that is refused (PP_EWORKSPACE), still no launch
    for kw in ({}, tex, {"colors": None, "base": grey}, {"base": grey}, dict(tex, base=grey), {"mode": 1, "nrm": p}, {"tone": p, "T": 2},
               {"tone": p, "T": 65536}, {"nl": 0, "lights": None}, {"nl": 0}, {"nl": 16, "lights": many}, {"ambient": 0.0}):
        assert lit(ws_bytes=one - 1, **kw) == -2, kw
    assert lit(ws=p + 64) == -2
