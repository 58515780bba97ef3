"""GPU: the lit render (pp_render_views_lit) and pp_vertex_normals bit-equal to tests/shading_oracle.py for every colour source,
normal mode, tone table and frame; identity shading equal to the unlit render; the untextured case the feature exists for; the
shaded bank; the unlit paths unchanged; determinism; and the argument checks with a device present."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_oracle as ro  # noqa: E402
import shading_oracle as so  # noqa: E402
import texture_oracle as to  # noqa: E402
from test_textured_bank_gpu import K_OBJ, _poses, _render, _same, _textured  # noqa: E402

from picopose_amd.provider import template_bank as tb  # noqa: E402

gpu = pytest.mark.gpu
H, W = to.FRAME
CONST = (90, 160, 230)


def _mesh(name, source):
    """cube / icosphere(2) with vertex colours, a texture, or neither (the constant base colour is given with the shading).  The
    cube carries normals of its own (random, not unit length); the icosphere's smooth normals come from pp_vertex_normals."""
    m = ro.cube(0.4) if name == "cube" else ro.icosphere(2, 0.5)
    if source == "texture":
        m = _textured(name, 21)
    elif source == "constant":
        m = {"vertices": m["vertices"], "faces": m["faces"]}
    else:
        m = dict(m)
    if name == "cube":
        m["normals"] = np.random.default_rng(7).normal(size=(8, 3)).astype(np.float32) * np.float32(3)
    return m


def _light_sets():
    t = tb.template_lights(1.5, "blenderproc", key=1.7)
    eight = {"lights": t["lights"], "intensity": t["intensity"], "ambient": 0.0}
    # one light at the side, one behind every object (the farthest pose is at z = 5), one of intensity 0 at the camera
    three = {"lights": [[2.5, 0.3, 1.6], [0.0, 0.0, 8.0], [0.0, 0.0, 0.0]], "intensity": [9.0, 40.0, 0.0], "ambient": 0.2}
    return {"blenderproc_eight": eight, "side_behind_zero": three}


def _lights4(ls):
    return np.concatenate([np.asarray(ls["lights"], dtype=np.float64), np.asarray(ls["intensity"], dtype=np.float64)[:, None]], axis=1).astype(np.float32)


def _oracle(mesh, poses, K, h, w, ls, smooth, base, tone):
    normals = None
    if smooth:
        normals = mesh["normals"] if mesh.get("normals") is not None else so.vertex_normals(mesh["vertices"], mesh["faces"])
    return so.render(mesh, poses.astype(np.float32), K, h, w, _lights4(ls), ls["ambient"], normals=normals, base_color=base,
                     tone=None if tone is None else tb.srgb_tone_table(4096))


# ---- 1. kernel == oracle ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("frame", ["whole", "odd_partly_outside_chunked"])
@pytest.mark.parametrize("tone", [None, "srgb"])
@pytest.mark.parametrize("normals", ["flat", "smooth"])
@pytest.mark.parametrize("source", ["vertex_colour", "texture", "constant"])
@pytest.mark.parametrize("name", ["cube", "icosphere"])
def test_lit_render_equals_the_oracle(name, source, normals, tone, frame):
    mesh = _mesh(name, source)
    base = CONST if source == "constant" else None
    if frame == "whole":
        h, w, kw = H, W, {}
        poses = _poses(22, 4, 0.1, [1.1, 1.6, 2.5, 5.0])
    else:                                                       # one view per chunk: four chunks
        h, w = 47, 61
        poses = _poses(23, 4, 0.55, [1.2, 1.5, 2.0, 3.0])
        kw = {"workspace_bytes": 256 + (h * w + len(mesh["faces"])) * 8}
    dark = saturated = False
    for ls in _light_sets().values():
        got = _render(mesh, poses, K_OBJ, h, w, shading=dict(ls, normals=normals, base_color=base, tone=tone), **kw)
        want = _oracle(mesh, poses, K_OBJ, h, w, ls, normals == "smooth", base, tone)
        _same(got, want)
        assert int(got["near_count"].item()) == want["near_count"] == 0
        cover = want["face_id"] >= 0
        assert cover.reshape(4, -1).sum(axis=1).min() > 40
        dark |= bool(ls["ambient"] > 0 and (want["s"][cover] == 0).any())
        saturated |= bool((want["rgba"][..., :3][cover] == 255).any())
        assert len(np.unique(want["s"][cover])) > 20                      # it is a shaded picture
    assert dark and saturated                                            # ambient-only samples and the clamp at 255 are both reached
    boxes = []
    for p in poses.astype(np.float32):
        t = ro.Triangles(mesh["vertices"], mesh["faces"], p, ro._k4(K_OBJ), h, w, 1e-3)
        boxes.append(((t.bx1 - t.bx0 + 1) * (t.by1 - t.by0 + 1))[t.keep])
    boxes = np.concatenate(boxes)
    assert (boxes > 64).any() if name == "cube" else ((boxes > 64).any() and (boxes <= 64).any())      # queued tiles / a lane's walk
    if frame != "whole":
        touching = sum(bool(c[0].any() or c[-1].any() or c[:, 0].any() or c[:, -1].any()) for c in cover)
        assert touching >= 2


# ---- 2. vertex normals -----------------------------------------------------------------------------------------------------------------
def _normal_meshes():
    c, s = ro.cube(0.4), ro.icosphere(2, 0.5)
    lone = {"vertices": np.concatenate([c["vertices"], np.float32([[9, 9, 9]])]), "faces": c["faces"]}
    flat = {"vertices": np.concatenate([s["vertices"], np.float32([[1, 2, 3]])]),
            "faces": np.concatenate([s["faces"], np.int32([[0, 0, 5], [3, len(s["vertices"]), 3], [7, 7, 7]])])}
    return {"cube": c, "icosphere": s, "unreferenced_vertex": lone, "zero_area_faces": flat}


@gpu
@pytest.mark.parametrize("name", ["cube", "icosphere", "unreferenced_vertex", "zero_area_faces"])
def test_vertex_normals_equal_the_oracle_on_any_stream(name):
    mesh = _normal_meshes()[name]
    want = so.vertex_normals(mesh["vertices"], mesh["faces"])
    a = tb.vertex_normals(mesh)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = tb.vertex_normals(mesh)
    torch.cuda.synchronize()
    assert a.dtype == torch.float32 and tuple(a.shape) == want.shape
    assert np.array_equal(a.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if name == "unreferenced_vertex":
        assert np.all(want[8] == 0) and np.all(np.abs(np.linalg.norm(want[:8], axis=1) - 1) < 1e-6)
    if name == "zero_area_faces":
        assert np.all(want[-1] == 0) and np.array_equal(want[:-1], so.vertex_normals(ro.icosphere(2, 0.5)["vertices"], ro.icosphere(2, 0.5)["faces"]))


# ---- 3. identity -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("source", ["vertex_colour", "texture"])
@pytest.mark.parametrize("normals", ["flat", "smooth"])
def test_no_lights_and_ambient_one_give_the_unlit_render(source, normals):
    """Pins "base colour = the unlit pixel": multiplying it by 1 changes no byte."""
    mesh = _mesh("icosphere", source)
    poses = _poses(32, 4, 0.2, [1.1, 1.5, 2.2, 4.0])
    unlit = _render(mesh, poses, K_OBJ, H, W)
    lit = _render(mesh, poses, K_OBJ, H, W, shading={"ambient": 1.0, "normals": normals})
    _same(lit, unlit)
    assert (unlit["rgba"][..., 3] == 255).sum() > 500 and len(torch.unique(unlit["rgba"][..., 0])) > 50


# ---- 4. the untextured model -----------------------------------------------------------------------------------------------------------
@gpu
def test_colourless_cube_shows_its_faces_only_when_shaded():
    c = ro.cube(0.4)
    mesh = {"vertices": c["vertices"], "faces": c["faces"]}
    poses = _poses(44, 4, 0.0, [tb.mesh_diameter(c["vertices"])] * 4)       # the distance "tless" sets its lights for; three sides show in each
    K = np.array([[90.0, 0, 31.5], [0, 88.0, 23.5], [0, 0, 1.0]])
    unlit = _render(mesh, poses, K, H, W)
    lit = _render(mesh, poses, K, H, W, shading="tless")
    _same(lit, unlit, keys=("depth_mm", "depth_m", "face_id"))
    for v in range(4):
        cover = unlit["face_id"][v] >= 0
        assert int(cover.sum()) > 200
        flat = torch.unique(unlit["rgba"][v][cover], dim=0)
        assert flat.tolist() == [[128, 128, 128, 255]]                      # unlit: one colour, a silhouette
        px = lit["rgba"][v][cover]
        assert torch.equal(px[:, 0], px[:, 1]) and torch.equal(px[:, 0], px[:, 2]) and bool((px[:, 3] == 255).all())      # grey
        assert len(torch.unique(px[:, 0])) >= 3
        side = (lit["face_id"][v][cover] // 2)                              # two triangles per side of the cube
        means = sorted(float(px[side == s, 0].float().mean()) for s in torch.unique(side).tolist() if int((side == s).sum()) >= 20)
        assert len(means) >= 2 and means[-1] - means[0] > 2.0, means


# ---- 5. the bank -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_shaded_bank_moves_colour_only(golden_dir):
    views = np.load(os.path.join(golden_dir, "template_view_poses_level1.npy"))[::45]      # 4 views
    K = np.array([[60.0, 0, 32.0], [0, 60.0, 24.0], [0, 0, 1.0]])
    kw = {"K": K, "resolution": (H, W), "units": "m", "img_size": 56, "pts_size": 16}
    c = ro.cube(0.4)
    mesh = {"vertices": c["vertices"], "faces": c["faces"]}
    plain = tb.render_templates(mesh, views, **kw)
    shaded = tb.render_templates(mesh, views, shading="tless", **kw)
    assert set(plain) == set(shaded)
    for k in ("tem_mask", "tem_pts3d", "tem_bbox", "tem_M", "tem_pose", "tem_K"):
        assert torch.equal(plain[k], shaded[k]), k
    assert not torch.equal(plain["tem_rgb"], shaded["tem_rgb"])
    poses = tb.template_object_poses(views, mesh["vertices"])
    frames = tb.render_views(mesh, poses, K=K, resolution=(H, W), units="m", shading="tless")
    poses_mm = poses.copy()
    poses_mm[:, :3, 3] *= 1000.0
    again = tb.templates_from_frames(frames["rgba"], frames["depth_mm"], K, poses_mm, img_size=56, pts_size=16)
    assert torch.equal(again["tem_rgb"], shaded["tem_rgb"]) and torch.equal(again["tem_mask"], shaded["tem_mask"])
    want = so.render(mesh, poses.astype(np.float32), K, H, W, *tb._parse_shading("tless", tb.mesh_diameter(mesh["vertices"]))[:2],
                     base_color=(102, 102, 102))
    _same(frames, want, keys=("rgba", "depth_mm"))


# ---- 6. the unlit paths ------------------------------------------------------------------------------------------------------------------
@gpu
def test_default_renders_are_what_the_raster_and_texture_oracles_pin():
    poses = _poses(62, 4, 0.3, [1.0, 1.4, 2.0, 3.0])
    m = ro.icosphere(2, 0.5)
    _same(_render(m, poses, K_OBJ, H, W), ro.render(m["vertices"], m["faces"], m["colors"], poses.astype(np.float32), K_OBJ, H, W))
    t = _textured("icosphere", 61)
    _same(_render(t, poses, K_OBJ, H, W), to.render(t["vertices"], t["faces"], t["face_uv"], t["texture"], poses.astype(np.float32), K_OBJ, H, W))
    _same(_render(dict(m, normals=np.ones((len(m["vertices"]), 3), np.float32)), poses, K_OBJ, H, W, shading=None), _render(m, poses, K_OBJ, H, W))


# ---- 7. determinism ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_lit_render_is_deterministic_across_runs_streams_and_chunks():
    mesh = _mesh("icosphere", "texture")
    poses = _poses(72, 4, 0.3, [1.0, 1.4, 2.0, 3.0])
    sh = dict(_light_sets()["side_behind_zero"], normals="smooth", tone="srgb")
    per_view = (H * W + len(mesh["faces"])) * 8
    base = _render(mesh, poses, K_OBJ, H, W, shading=sh)
    again = _render(mesh, poses, K_OBJ, H, W, shading=sh)
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        side = _render(mesh, poses, K_OBJ, H, W, shading=sh, workspace_bytes=256 + 3 * per_view)       # 2 chunks on a side stream
    one = _render(mesh, poses, K_OBJ, H, W, shading=sh, workspace_bytes=0)                             # 4 chunks
    torch.cuda.synchronize()
    for other in (again, side, one):
        _same(other, base)
    assert len(torch.unique(base["rgba"][..., 0])) > 30


# ---- 8. argument validation ------------------------------------------------------------------------------------------------------------------
@gpu
def test_shading_entries_refuse_bad_arguments_before_any_launch():
    """The checks of tests/test_shaded_bank_cpu.py with a device present: every call returns its error code from the host-side
    checks, nothing is enqueued, and the stream goes on working."""
    from test_shaded_bank_cpu import test_shading_abi_argument_validation_needs_no_gpu as checks

    torch.cuda.synchronize()
    checks()
    torch.cuda.synchronize()
    assert int(torch.arange(5, device="cuda").sum().item()) == 10
