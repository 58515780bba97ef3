"""CPU: the texture oracle (tests/texture_oracle.py) against closed-form answers that do not come from it, so that the GPU tests of
tests/test_textured_bank_gpu.py inherit a trusted yardstick; the host side of textured onboarding in
picopose_amd/provider/template_bank.py (load_ply's UVs, load_texture, load_model, the mesh-dict validation); and the argument checks
of pp_texture_mips_bytes / pp_texture_build_mips / pp_render_views_textured through the ABI (no GPU)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_oracle as ro  # noqa: E402
import texture_oracle as to  # noqa: E402

from picopose_amd.provider import template_bank as tb  # noqa: E402

H, W = to.FRAME


def _quad_view(tex, x0, y0, wpx, hpx, uv_shift=(0.0, 0.0), faces=None, face_uv=None):
    v, f, uv = to.screen_quad(x0, y0, wpx, hpx)
    fuv = to.expand_uv(uv + np.float32(uv_shift), f) if face_uv is None else face_uv
    return to.render_view(v, f if faces is None else faces, fuv, tex, to.pose(), to.K_SMALL, H, W)


# ---- 1. the pyramid --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,want", [((16, 8), [(16, 8), (8, 4), (4, 2), (2, 1), (1, 1)]), ((12, 6), [(12, 6), (6, 3), (3, 1), (1, 1)]),
                                        ((5, 3), [(5, 3), (2, 1), (1, 1)]), ((1, 7), [(1, 7), (1, 3), (1, 1)])])
def test_pyramid_levels_and_sizes(size, want):
    Wt, Ht = size
    levels = to.build_mips(to.random_texture(Wt, Ht, 1))
    assert [(lv.shape[1], lv.shape[0]) for lv in levels] == want and all(lv.dtype == np.uint8 and lv.shape[2] == 3 for lv in levels)
    const = to.build_mips(np.full((Ht, Wt, 3), [7, 200, 255], dtype=np.uint8))
    assert all(np.all(lv == [7, 200, 255]) for lv in const)                  # (4 c + 2) >> 2 = c
    assert to.pack_mips(levels).shape == (sum(w * h for w, h in want), 4) and np.all(to.pack_mips(levels)[:, 3] == 255)


def test_pyramid_hand_computed_4x2_and_odd_sizes():
    img = np.zeros((2, 4, 3), dtype=np.uint8)
    img[..., 0] = [[0, 1, 10, 20], [2, 4, 30, 41]]                           # (0+1+2+4+2)>>2 = 2, (10+20+30+41+2)>>2 = 25
    img[..., 1] = [[255, 255, 0, 0], [255, 254, 0, 1]]                       # (1019+2)>>2 = 255, (1+2)>>2 = 0
    img[..., 2] = [[3, 3, 3, 4], [3, 3, 4, 4]]                               # (12+2)>>2 = 3, (15+2)>>2 = 4
    l0, l1, l2 = to.build_mips(img)
    assert l1.tolist() == [[[2, 255, 3], [25, 0, 4]]]
    assert l2.tolist() == [[[(2 + 25 + 2 + 25 + 2) >> 2, (255 + 0 + 255 + 0 + 2) >> 2, (3 + 4 + 3 + 4 + 2) >> 2]]]      # the row tap is clamped: counted twice
    odd = np.arange(15, dtype=np.uint8).reshape(3, 5, 1).repeat(3, axis=2)   # 5 x 3 -> 2 x 1: rows 0-1, columns 0-1 | 2-3 (column 4 and row 2 dropped)
    assert to.build_mips(odd)[1][..., 0].tolist() == [[(0 + 1 + 5 + 6 + 2) >> 2, (2 + 3 + 7 + 8 + 2) >> 2]]
    col = np.array([10, 20, 30, 40, 50, 60, 70], dtype=np.uint8).reshape(7, 1, 1).repeat(3, axis=2)      # 1 x 7 -> 1 x 3: the column tap is clamped
    assert to.build_mips(col)[1][..., 0].ravel().tolist() == [(10 + 10 + 20 + 20 + 2) >> 2, (30 + 30 + 40 + 40 + 2) >> 2, (50 + 50 + 60 + 60 + 2) >> 2]


# ---- 2.-3. identity mapping and exact minification ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 8), (12, 6)])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_quad_with_texel_centres_on_pixel_centres_reproduces_the_mip_level(size, level):
    """The quad covers Wt/2^l x Ht/2^l pixels with its edges half a pixel outside, so pixel (x0 + i, y0 + j) has u = (i + 1/2) / W_l,
    v = 1 - (j + 1/2) / H_l in real arithmetic: T5's x = i, y = j, the centre of texel (i, j) of level l — row 0 at the TOP (the v
    flip), column 0 at the LEFT.  T3: per triangle A_t = Wt Ht and A_p = (Wt >> l)(Ht >> l) >= A_t / (1.5 4^l), so the level is l
    (A_t <= 2 A_p 4^l, and A_t > 2 A_p 4^(l-1) since A_p <= A_t / 4^l).  float32 moves x by a few 1e-6: the sample is texel (i, j)
    blended with a neighbour at weight <= 1e-5, less than 0.003 grey levels from the texel, so the rounded byte is the texel exactly."""
    Wt, Ht = size
    tex = to.random_texture(Wt, Ht, 3)
    want = to.build_mips(tex)[level]
    hpx, wpx = want.shape[:2]
    assert (wpx, hpx) == (Wt >> level, Ht >> level)
    x0, y0 = 9, 5
    r = _quad_view(tex, x0, y0, wpx, hpx)
    cover = np.zeros((H, W), bool)
    cover[y0:y0 + hpx, x0:x0 + wpx] = True
    assert np.array_equal(r["face_id"] >= 0, cover) and np.all(r["level"][cover] == level)
    assert np.array_equal(r["rgba"][y0:y0 + hpx, x0:x0 + wpx, :3], want) and np.all(r["rgba"][cover][:, 3] == 255)
    assert np.all(r["rgba"][~cover] == 0) and np.all(r["depth_mm"][cover] == 2000)


# ---- 4. magnification ------------------------------------------------------------------------------------------------------------
def test_two_texels_across_four_pixels_give_the_bilinear_values():
    """Wt = 2, Ht = 1 over 4 x 2 pixels: u = (i + 1/2) / 4, x = 2 u - 1/2 = -1/4, 1/4, 3/4, 5/4.  x = -1/4: taps -1 -> 1 (repeat) and 0
    with fx = 3/4; x = 5/4: taps 1 and 2 -> 0 with fx = 1/4.  Texels (40, 0, 255) and (200, 100, 255):
    red 200 - 120 = 80, 40 + 40 = 80, 40 + 120 = 160, 200 - 40 = 160; green 25, 25, 75, 75.  Ht = 1: both row taps are row 0."""
    tex = np.array([[[40, 0, 255], [200, 100, 255]]], dtype=np.uint8)
    r = _quad_view(tex, 20, 10, 4, 2)
    assert np.all(r["level"][10:12, 20:24] == 0)
    for row in r["rgba"][10:12, 20:24]:
        assert row.tolist() == [[80, 25, 255, 255], [80, 25, 255, 255], [160, 75, 255, 255], [160, 75, 255, 255]]


# ---- 5.-7. repeat, winding, layout -------------------------------------------------------------------------------------------------
def test_uvs_shifted_by_whole_periods_give_the_same_frame():
    tex = to.random_texture(16, 8, 4)
    base = _quad_view(tex, 9, 5, 16, 8)
    moved = _quad_view(tex, 9, 5, 16, 8, uv_shift=(1.0, -2.0))
    for k in ("rgba", "depth_mm", "face_id", "level"):
        assert np.array_equal(base[k], moved[k]), k


def _random_cube(seed, Wt=12, Ht=6):
    m = ro.cube(0.4)
    rng = np.random.default_rng(seed)
    return m["vertices"], m["faces"], rng.uniform(-1.5, 2.5, (12, 3, 2)).astype(np.float32), to.random_texture(Wt, Ht, seed)


def _cube_pose(a=0.7, b=0.5, t=(0.05, -0.03, 2.2)):
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return to.pose(Rx @ Ry, t)


K_CUBE = np.array([[60.0, 0, 31.5], [0, 58.0, 23.5], [0, 0, 1.0]])


def test_winding_does_not_change_the_frame():
    """Corners 1 and 2 exchanged together with their UVs: item 4 orders both windings into the same triangle, the determinant of T3
    is negated exactly, so every bit is the same.  On the identity quad any exchange (here 0 and 1) gives the same bytes too."""
    v, f, fuv, tex = _random_cube(5)
    a = to.render_view(v, f, fuv, tex, _cube_pose(), K_CUBE, H, W)
    b = to.render_view(v, f[:, [0, 2, 1]], fuv[:, [0, 2, 1]], tex, _cube_pose(), K_CUBE, H, W)
    assert (a["face_id"] >= 0).sum() > 300 and len(np.unique(a["face_id"])) >= 4
    for k in ("rgba", "depth_m", "face_id", "level"):
        assert np.array_equal(a[k], b[k]), k
    tex = to.random_texture(16, 8, 6)
    qv, qf, quv = to.screen_quad(9, 5, 16, 8)
    c = _quad_view(tex, 9, 5, 16, 8)
    d = _quad_view(tex, 9, 5, 16, 8, faces=qf[:, [1, 0, 2]], face_uv=to.expand_uv(quv, qf)[:, [1, 0, 2]])
    assert np.array_equal(c["rgba"], d["rgba"]) and np.array_equal(c["level"], d["level"])


def test_per_vertex_and_per_corner_uvs_give_the_same_frame():
    m = ro.icosphere(1, 0.5)
    rng = np.random.default_rng(8)
    uv = rng.uniform(-0.5, 1.5, (len(m["vertices"]), 2)).astype(np.float32)
    tex = to.random_texture(12, 6, 8)
    image, fuv = tb._mesh_texture({"vertices": m["vertices"], "texture": tex, "uv": uv}, len(m["vertices"]), m["faces"])
    assert fuv.dtype == np.float32 and fuv.shape == (80, 3, 2) and np.array_equal(fuv, to.expand_uv(uv, m["faces"])) and image is not None
    image2, fuv2 = tb._mesh_texture({"texture": tex, "uv": uv * 0, "face_uv": fuv.astype(np.float64)}, len(m["vertices"]), m["faces"])
    assert fuv2.dtype == np.float32 and np.array_equal(fuv2, fuv)            # face_uv wins over uv
    a = to.render_view(m["vertices"], m["faces"], fuv, tex, _cube_pose(), K_CUBE, H, W)
    b = to.render_view(m["vertices"], m["faces"], fuv2, tex, _cube_pose(), K_CUBE, H, W)
    assert (a["face_id"] >= 0).sum() > 300 and np.array_equal(a["rgba"], b["rgba"])


# ---- 8. perspective --------------------------------------------------------------------------------------------------------------
def test_tilted_quad_is_perspective_correct_and_affine_is_not():
    """A 2 x 1 quad turned 60 degrees about the camera's y axis at Zc = 2 (its ends at Zc = 1.13 and 2.87), f = 64 px, carrying a
    16 x 2 ramp g(i) = 10 + 15 i magnified 2.5 to 15 times.  Between texel centres bilinear filtering IS the linear ramp
    g(u) = 10 + 15 (16 u - 1/2), so for 1/16 <= u <= 15/16 (one texel from the seam, where the repeat wrap blends 235 with 10) the
    float64 answer is g(u) at the point where the pixel's ray meets the quad's plane.
    Error budget against it, in grey levels: the byte rounding, 0.5; the 1/512 px vertex snap, which moves the image of the ramp by
    that much: the ramp is steepest at the far end, where neighbouring pixels differ by at most 16 levels (asserted below on the
    float64 answer), so 16 / 512 = 0.03; float32 in the weights and the division: 8 u relative on values <= 255 and on 16 u:
    < 0.001.  Total < 0.54: the bound of 1 level holds with room, and a wrong interpolation cannot hide in it: screen-space (affine)
    interpolation of the same UVs is off by about 240 (1/2 - 1.13 / (1.13 + 2.87)) = 52 levels mid-quad (the point halfway in the
    image is not halfway on the quad); asserted > 3."""
    th = np.deg2rad(60.0)
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    K = np.array([[64.0, 0, 32.0], [0, 64.0, 24.0], [0, 0, 1.0]])
    v = np.array([[-1, -0.5, 0], [1, -0.5, 0], [-1, 0.5, 0], [1, 0.5, 0]], dtype=np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2]], dtype=np.int32)
    fuv = to.expand_uv(np.array([[0, 1], [1, 1], [0, 0], [1, 0]], dtype=np.float32), f)
    tex = np.zeros((2, 16, 3), dtype=np.uint8)
    tex[:] = (10 + 15 * np.arange(16))[None, :, None]
    P = to.pose(R, (0, 0, 2.0))
    r = to.render_view(v, f, fuv, tex, P, K, H, W)
    cover = r["face_id"] >= 0
    assert cover.sum() > 400 and np.all(r["level"][cover] == 0)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(xx - 32) / 64.0, (yy - 24) / 64.0, np.ones((H, W))], axis=-1)      # rays through the pixel centres
    t = np.array([0, 0, 2.0])
    s = (R[:, 2] @ t) / (d @ R[:, 2])
    obj = (d * s[..., None] - t) @ R                                          # R^T (X - t)
    u = (obj[..., 0] + 1) / 2
    assert np.abs(obj[..., 2][cover]).max() < 1e-12
    inner = cover & (u >= 1 / 16) & (u <= 15 / 16)
    want = 10 + 15 * (16 * u - 0.5)
    per_px = np.abs(np.diff(want, axis=1))[inner[:, 1:] & inner[:, :-1]].max()
    assert inner.sum() > 300 and per_px <= 16
    err = np.abs(r["rgba"][..., 0].astype(np.float64) - want)[inner]
    print("perspective: max error", err.max(), "levels; steepest ramp", per_px, "levels per pixel")
    assert err.max() <= 1.0 and np.all(r["rgba"][..., 1][inner] == r["rgba"][..., 0][inner])
    a = to.render_view(v, f, fuv, tex, P, K, H, W, affine=True)
    off = np.abs(a["rgba"][..., 0].astype(np.float64) - want)[inner]
    print("affine: max error", off.max())
    assert off.max() > 3.0


# ---- 9. constant texture -----------------------------------------------------------------------------------------------------------
def test_constant_texture_equals_the_vertex_colour_render():
    v, f, fuv, _ = _random_cube(9)
    C = np.array([37, 200, 255], dtype=np.uint8)
    tex = np.full((16, 32, 3), C, dtype=np.uint8)
    a = to.render_view(v, f, fuv, tex, _cube_pose(), K_CUBE, H, W)
    b = ro.render_view(v, f, np.tile(C, (8, 1)), _cube_pose(), K_CUBE, H, W)
    for k in ("rgba", "depth_mm", "depth_m", "face_id"):
        assert np.array_equal(a[k], b[k]), k
    assert len(np.unique(a["level"][a["level"] >= 0])) >= 2                   # through more than one mip level


# ---- 10. loaders -------------------------------------------------------------------------------------------------------------------
def _write_textured_ply(path, v, f, binary, uv=None, uv_names=("texture_u", "texture_v"), face_uv=None, texture_file=None, texnumber=False,
                        bad_face=None):
    head = ["ply", "format binary_little_endian 1.0" if binary else "format ascii 1.0", "comment made by a test"]
    if texture_file:
        head.append(f"comment TextureFile {texture_file}")
    head += [f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    if uv is not None:
        head += [f"property float {uv_names[0]}", f"property float {uv_names[1]}"]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices"]
    if face_uv is not None:
        head.append("property list uchar float texcoord")
    if texnumber:
        head.append("property int texnumber")
    head.append("end_header")
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        vt = np.concatenate([v, uv], axis=1).astype("<f4") if uv is not None else v.astype("<f4")
        if binary:
            fh.write(vt.tobytes())
        else:
            fh.write(("\n".join(" ".join(repr(float(x)) for x in row) for row in vt) + "\n").encode("ascii"))
        for k, tri in enumerate(f):
            tc = [] if face_uv is None else [float(x) for x in face_uv[k].ravel()]
            if bad_face == k:
                tc = tc[:4]
            if binary:
                fh.write(b"\x03" + np.asarray(tri, "<i4").tobytes())
                if face_uv is not None:
                    fh.write(bytes([len(tc)]) + np.asarray(tc, "<f4").tobytes())
                if texnumber:
                    fh.write(np.asarray([0], "<i4").tobytes())
            else:
                row = ["3"] + [str(int(i)) for i in tri] + ([str(len(tc))] + [repr(x) for x in tc] if face_uv is not None else [])
                fh.write((" ".join(row + (["0"] if texnumber else [])) + "\n").encode("ascii"))


@pytest.mark.parametrize("binary", [False, True])
def test_load_ply_reads_uvs_and_the_texture_name(tmp_path, binary):
    m = ro.icosphere(1, 37.5)
    v, f = m["vertices"], m["faces"]
    rng = np.random.default_rng(12)
    uv = rng.uniform(-1, 2, (len(v), 2)).astype(np.float32)
    fuv = rng.uniform(-1, 2, (len(f), 3, 2)).astype(np.float32)
    p = str(tmp_path / "m.ply")
    for names in (("texture_u", "texture_v"), ("s", "t"), ("u", "v")):
        _write_textured_ply(p, v, f, binary, uv=uv, uv_names=names, texture_file="obj_000001.png")
        got = tb.load_ply(p)
        assert np.array_equal(got["vertices"], v) and np.array_equal(got["faces"], f) and got["colors"] is None
        assert got["uv"].dtype == np.float32 and np.array_equal(got["uv"], uv) and got["face_uv"] is None
        assert got["texture_file"] == "obj_000001.png"
    for texnumber in (False, True):
        _write_textured_ply(p, v, f, binary, face_uv=fuv, texnumber=texnumber, texture_file="a b.png")
        got = tb.load_ply(p)
        assert np.array_equal(got["faces"], f) and got["faces"].dtype == np.int32 and got["uv"] is None
        assert got["face_uv"].dtype == np.float32 and got["face_uv"].shape == (len(f), 3, 2) and np.array_equal(got["face_uv"], fuv)
        assert got["texture_file"] == "a b.png"
    _write_textured_ply(p, v, f, binary)
    got = tb.load_ply(p)
    assert got["uv"] is None and got["face_uv"] is None and got["texture_file"] is None and np.array_equal(got["faces"], f)
    _write_textured_ply(p, v, f, binary, face_uv=fuv, texnumber=True, bad_face=5)
    with pytest.raises(ValueError, match="face 5 holds a texcoord list of 4"):
        tb.load_ply(p)


def test_load_texture_and_load_model_round_trip(tmp_path):
    from PIL import Image

    m = ro.cube(10.0)
    rng = np.random.default_rng(13)
    uv = rng.uniform(0, 1, (8, 2)).astype(np.float32)
    rgb = to.random_texture(12, 6, 13)
    Image.fromarray(rgb).save(str(tmp_path / "rgb.png"))
    rgba = np.concatenate([rgb, rng.integers(0, 256, (6, 12, 1)).astype(np.uint8)], axis=2)
    Image.fromarray(rgba).save(str(tmp_path / "rgba.png"))
    pal = rng.integers(0, 4, (6, 12)).astype(np.uint8)
    colours = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [9, 99, 199]], dtype=np.uint8)
    im = Image.new("P", (12, 6))
    im.putdata(pal.ravel().tolist())
    im.putpalette(colours.ravel().tolist() + [0] * (768 - 12))
    im.save(str(tmp_path / "pal.png"))
    for name, want in (("rgb.png", rgb), ("rgba.png", rgb), ("pal.png", colours[pal])):
        got = tb.load_texture(str(tmp_path / name))
        assert got.dtype == np.uint8 and got.shape == (6, 12, 3) and got.flags.c_contiguous and np.array_equal(got, want), name
        ply = str(tmp_path / "m.ply")
        _write_textured_ply(ply, m["vertices"], m["faces"], True, uv=uv, texture_file=name)
        mesh = tb.load_model(ply)
        assert np.array_equal(mesh["texture"], want) and np.array_equal(mesh["uv"], uv) and mesh["texture_file"] == name
        image, fuv = tb._mesh_texture(mesh, 8, mesh["faces"])
        assert np.array_equal(image, want) and np.array_equal(fuv, uv[m["faces"]])
    ply = str(tmp_path / "n.ply")
    _write_textured_ply(ply, m["vertices"], m["faces"], False, uv=uv, texture_file="missing.png")
    with pytest.raises(ValueError, match="missing.png"):
        tb.load_model(ply)
    with pytest.raises(ValueError, match="nowhere.png"):
        tb.load_model(ply, texture=str(tmp_path / "nowhere.png"))
    assert np.array_equal(tb.load_model(ply, texture=str(tmp_path / "rgb.png"))["texture"], rgb)      # the argument wins over the comment
    assert np.array_equal(tb.load_model(ply, texture=rgb[::-1])["texture"], rgb[::-1])
    _write_textured_ply(ply, m["vertices"], m["faces"], False)
    assert "texture" not in tb.load_model(ply)                               # no UVs, no texture: load_ply's result


def test_mesh_dict_validation_of_texture_and_uvs():
    m = ro.cube(10.0)
    v, f = m["vertices"], m["faces"]
    tex = to.random_texture(12, 6, 14)
    uv = np.zeros((8, 2), np.float32)
    assert tb._mesh_texture({"vertices": v, "faces": f, "uv": uv}, 8, f) is None          # no texture: today's path
    for bad, match in (({"texture": tex}, "needs 'face_uv'"), ({"texture": tex, "uv": np.zeros((7, 2), np.float32)}, r"uv must be a \(Nv, 2\)"),
                       ({"texture": tex, "uv": np.zeros((8, 2), np.int32)}, "uv must be"),
                       ({"texture": tex, "face_uv": np.zeros((12, 3, 3), np.float32)}, r"face_uv must be a \(Nf, 3, 2\)"),
                       ({"texture": tex, "face_uv": np.zeros((11, 3, 2), np.float32)}, "face_uv must be"),
                       ({"texture": tex, "uv": np.full((8, 2), np.nan, np.float32)}, "non-finite"),
                       ({"texture": tex, "face_uv": np.full((12, 3, 2), np.inf)}, "non-finite"),
                       ({"texture": tex.astype(np.float32), "uv": uv}, "texture must be"), ({"texture": tex[..., 0], "uv": uv}, "texture must be"),
                       ({"texture": np.zeros((6, 12, 4), np.uint8), "uv": uv}, "texture must be"),
                       ({"texture": np.zeros((0, 12, 3), np.uint8), "uv": uv}, "texture must be")):
        with pytest.raises(ValueError, match=match):
            tb._mesh_texture(dict(bad, vertices=v, faces=f), 8, f)


# ---- the C ABI's argument checks (they run before any launch: no GPU) ----------------------------------------------------------------
def test_texture_abi_argument_validation_needs_no_gpu():
    from picopose_amd import _lib

    L = _lib.lib()
    assert {"pp_texture_mips_bytes", "pp_texture_build_mips", "pp_render_views_textured"} <= set(_lib.declared_symbols())
    need, levels = ctypes.c_size_t(), ctypes.c_int()
    for (Wt, Ht), texels, n in (((16, 8), 171, 5), ((12, 6), 72 + 18 + 3 + 1, 4), ((5, 3), 15 + 2 + 1, 3), ((1, 7), 7 + 3 + 1, 3),
                                ((1, 1), 1, 1), ((16384, 16384), (4 ** 15 - 1) // 3, 15)):
        assert L.pp_texture_mips_bytes(Wt, Ht, ctypes.byref(need), ctypes.byref(levels)) == 0
        assert (need.value, levels.value) == (4 * texels, n), (Wt, Ht)
    assert L.pp_texture_mips_bytes(16, 8, ctypes.byref(need), None) == 0 and need.value == 684
    for Wt, Ht in ((0, 8), (16, 0), (-1, 8), (16385, 8), (16, 16385)):
        assert L.pp_texture_mips_bytes(Wt, Ht, ctypes.byref(need), None) == -1
    assert L.pp_texture_mips_bytes(16, 8, None, ctypes.byref(levels)) == -1
    buf = (ctypes.c_char * 2048)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256

    def mips(rgb=p, Wt=16, Ht=8, out=p, nbytes=684):
        return L.pp_texture_build_mips(rgb, Wt, Ht, out, nbytes, None)

    for kw in ({"rgb": None}, {"out": None}, {"Wt": 0}, {"Ht": 0}, {"Wt": 16385}, {"out": p + 2}, {"out": p + 1}, {"nbytes": 683}, {"nbytes": 0}):
        assert mips(**kw) == -1, kw
    i32 = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    one = 256 + (480 * 640 + 2) * 8

    def render(verts=p, nv=4, faces=p, faces_h=i32(0, 1, 2, 0, 2, 3), nf=2, uv=p, mip=p, Wt=16, Ht=8, poses=p, V=3, fx=500.0, fy=500.0,
               H=480, W=640, near=1e-3, ws=p, ws_bytes=one, rgba=p, dmm=p, cnt=p):
        return L.pp_render_views_textured(verts, nv, faces, faces_h, nf, uv, mip, Wt, Ht, poses, V, fx, fy, 320.0, 240.0, H, W, near, ws,
                                          ws_bytes, rgba, dmm, None, None, cnt, None)

    for kw in ({"verts": None}, {"faces": None}, {"faces_h": None}, {"uv": None}, {"mip": None}, {"poses": None}, {"ws": None},
               {"rgba": None}, {"dmm": None}, {"cnt": None}, {"nv": 0}, {"nf": 0}, {"V": 0}, {"H": 0}, {"W": 0}, {"H": 50000, "W": 50000},
               {"near": 0.0}, {"fx": 0.0}, {"fy": 0.0}, {"Wt": 0}, {"Ht": 0}, {"Wt": 16385}, {"Ht": -3}, {"mip": p + 2}, {"uv": p + 1},
               {"rgba": p + 2}, {"faces_h": i32(0, 1, 2, 0, 2, 4)}, {"faces_h": i32(0, -1, 2, 0, 2, 3)}):
        assert render(**kw) == -1, kw
    assert render(ws_bytes=one - 1) == -2 and render(ws_bytes=0) == -2 and render(ws=p + 64) == -2      # PP_EWORKSPACE
