"""GPU: the textured render (pp_texture_build_mips + pp_render_views_textured) bit-equal to tests/texture_oracle.py, known answers on
the device that bypass the oracle, the untextured path unchanged, determinism, the bank of a textured mesh, and the argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_oracle as ro  # noqa: E402
import texture_oracle as to  # noqa: E402

from picopose_amd import _lib  # noqa: E402
from picopose_amd.provider import template_bank as tb  # noqa: E402

gpu = pytest.mark.gpu
H, W = to.FRAME
K_OBJ = np.array([[60.0, 0, 31.5], [0, 58.0, 23.5], [0, 0, 1.0]])
OUT = ("rgba", "depth_mm", "depth_m", "face_id")


def _textured(name, seed):
    """A cube (12 large triangles) or a 320-triangle icosphere with a random non-square texture and random per-corner UVs that leave
    [0, 1], scaled per face by 1/4 ... 8 in turn so that the faces of one frame fall on several mip levels; every 50th face from
    face 3 on has zero UV area."""
    m = ro.cube(0.4) if name == "cube" else ro.icosphere(2, 0.5)
    rng = np.random.default_rng(seed)
    nf = len(m["faces"])
    fuv = rng.uniform(-0.5, 0.5, (nf, 3, 2)) * 2.0 ** (np.arange(nf) % 6 - 2)[:, None, None] + rng.uniform(-1.5, 1.5, (nf, 1, 2))
    fuv[3::50] = fuv[3::50, :1]
    Wt, Ht = (32, 16) if name == "cube" else (12, 6)
    return {"vertices": m["vertices"], "faces": m["faces"], "face_uv": fuv.astype(np.float32), "texture": to.random_texture(Wt, Ht, seed)}


def _poses(seed, n, xy, z):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    poses = np.tile(np.eye(4), (n, 1, 1))
    poses[:, :3, :3] = q * np.sign(np.linalg.det(q))[:, None, None]
    poses[:, :3, 3] = np.stack([rng.uniform(-xy, xy, n), rng.uniform(-xy, xy, n), np.asarray(z, dtype=np.float64)], axis=1)
    return poses


def _render(mesh, poses, K, h, w, **kw):
    return tb.render_views(mesh, poses, K=K, resolution=(h, w), units="m", return_depth_m=True, return_face_id=True, check_near=False, **kw)


def _same(got, want, keys=OUT):
    for k in keys:
        a, b = got[k].cpu(), torch.from_numpy(want[k]) if isinstance(want[k], np.ndarray) else want[k].cpu()
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k


# ---- 1. kernel == oracle ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("frame", ["whole", "odd_partly_outside_chunked"])
@pytest.mark.parametrize("name", ["cube", "icosphere"])
def test_textured_render_equals_the_oracle(name, frame):
    mesh = _textured(name, 21)
    if frame == "whole":
        h, w, kw = H, W, {}
        poses = _poses(22, 4, 0.1, [1.1, 1.6, 2.5, 5.0])
    else:                                                       # one view per chunk: four chunks
        h, w = 47, 61
        poses = _poses(23, 4, 0.55, [1.2, 1.5, 2.0, 3.0])
        kw = {"workspace_bytes": 256 + (h * w + len(mesh["faces"])) * 8}
    got = _render(mesh, poses, K_OBJ, h, w, **kw)
    want = to.render(mesh["vertices"], mesh["faces"], mesh["face_uv"], mesh["texture"], poses.astype(np.float32), K_OBJ, h, w)
    _same(got, want)
    assert int(got["near_count"].item()) == want["near_count"] == 0
    cover = want["face_id"] >= 0
    assert cover.reshape(4, -1).sum(axis=1).min() > 40
    levels = [set(np.unique(lv[lv >= 0]).tolist()) for lv in want["level"]]
    # at least three mip levels in one frame (the cube cut by the odd frame shows fewer faces: two)
    assert max(len(s) for s in levels) >= (2 if (name, frame) == ("cube", "odd_partly_outside_chunked") else 3), levels
    flat = np.isin(want["face_id"], np.arange(3, len(mesh["faces"]), 50))
    assert flat.sum() >= 10 and np.all(want["level"][flat] == 0)             # faces without UV area are seen: level 0
    boxes = []
    for p in poses.astype(np.float32):
        t = ro.Triangles(mesh["vertices"], mesh["faces"], p, ro._k4(K_OBJ), h, w, 1e-3)
        boxes.append(((t.bx1 - t.bx0 + 1) * (t.by1 - t.by0 + 1))[t.keep])
    boxes = np.concatenate(boxes)
    assert (boxes > 64).any() if name == "cube" else ((boxes > 64).any() and (boxes <= 64).any())      # queued tiles / a lane's walk
    if frame != "whole":
        touching = sum(bool(c[0].any() or c[-1].any() or c[:, 0].any() or c[:, -1].any()) for c in cover)
        assert touching >= 2


# ---- 2. the pyramid --------------------------------------------------------------------------------------------------------------------
def _device_mips(tex):
    L = _lib.lib()
    Ht, Wt = tex.shape[:2]
    need, levels = ctypes.c_size_t(), ctypes.c_int()
    _lib.check(L.pp_texture_mips_bytes(Wt, Ht, ctypes.byref(need), ctypes.byref(levels)), "pp_texture_mips_bytes")
    rgb = torch.from_numpy(tex).cuda()
    mips = torch.full((need.value,), 77, dtype=torch.uint8, device="cuda")
    _lib.check(L.pp_texture_build_mips(rgb.data_ptr(), Wt, Ht, mips.data_ptr(), mips.numel(), _lib.stream_ptr()), "pp_texture_build_mips")
    return mips.cpu().numpy().reshape(-1, 4), levels.value


@gpu
@pytest.mark.parametrize("size", [(16, 8), (12, 6), (5, 3), (1, 7)])
def test_device_pyramid_equals_the_oracle(size):
    tex = to.random_texture(*size, seed=31)
    want = to.build_mips(tex)
    got, n = _device_mips(tex)
    assert n == len(want) and np.array_equal(got, to.pack_mips(want))


# ---- 3. known answers on the device (not through the oracle) ---------------------------------------------------------------------------
def _halve(t):
    """The next mip level of an image whose sides are even or 1, written independently of the oracle: the rounded mean of 2 x 2
    blocks (of 2 x 1 / 1 x 2 blocks counted twice for a side of 1)."""
    t = t.astype(np.int64)
    if t.shape[0] == 1:
        t = np.concatenate([t, t], axis=0)
    if t.shape[1] == 1:
        t = np.concatenate([t, t], axis=1)
    h, w = t.shape[0] // 2, t.shape[1] // 2
    return ((t[:2 * h, :2 * w].reshape(h, 2, w, 2, 3).sum(axis=(1, 3)) + 2) >> 2).astype(np.uint8)


def _quad_mesh(tex, x0, y0, wpx, hpx, uv_shift=(0.0, 0.0)):
    v, f, uv = to.screen_quad(x0, y0, wpx, hpx)
    return {"vertices": v, "faces": f, "uv": uv + np.float32(uv_shift), "texture": tex}


@gpu
@pytest.mark.parametrize("size", [(16, 8), (12, 6)])
def test_device_identity_and_exact_minification(size):
    """CPU cases 2 and 3 (tests/test_textured_bank_cpu.py states the derivation): texel centres on pixel centres reproduce the
    texture at full size and mip levels 1 and 2 at half and quarter size, upright and unmirrored."""
    Wt, Ht = size
    tex = to.random_texture(Wt, Ht, 3)
    want = tex
    for level in range(3):
        hpx, wpx = want.shape[:2]
        assert (wpx, hpx) == (Wt >> level, Ht >> level)
        r = _render(_quad_mesh(tex, 9, 5, wpx, hpx), to.pose()[None], to.K_SMALL, H, W)
        rgba = r["rgba"][0].cpu().numpy()
        cover = np.zeros((H, W), bool)
        cover[5:5 + hpx, 9:9 + wpx] = True
        assert np.array_equal(rgba[..., 3] == 255, cover) and np.all(rgba[~cover] == 0), level
        assert np.array_equal(rgba[5:5 + hpx, 9:9 + wpx, :3], want), level
        assert np.all(r["depth_mm"][0].cpu().numpy()[cover] == 2000)
        want = _halve(want[:want.shape[0] - (want.shape[0] % 2 if want.shape[0] > 1 else 0)])       # (6 x 3 -> 3 x 1 uses rows 0 and 1)


@gpu
def test_device_repeat_winding_and_constant_texture():
    """CPU cases 5, 6 and 9 on the device: UVs moved by (+1, -2) and exchanged corners give the same frame; a constant texture gives
    the vertex-colour entry's bytes for that colour."""
    tex = to.random_texture(16, 8, 4)
    base = _render(_quad_mesh(tex, 9, 5, 16, 8), to.pose()[None], to.K_SMALL, H, W)
    assert np.array_equal(base["rgba"][0, 5:13, 9:25, :3].cpu().numpy(), tex)
    _same(_render(_quad_mesh(tex, 9, 5, 16, 8, uv_shift=(1.0, -2.0)), to.pose()[None], to.K_SMALL, H, W), base)
    q = _quad_mesh(tex, 9, 5, 16, 8)
    fuv = to.expand_uv(q["uv"], q["faces"])
    _same(_render({"vertices": q["vertices"], "faces": q["faces"][:, [1, 0, 2]], "face_uv": fuv[:, [1, 0, 2]], "texture": tex},
                  to.pose()[None], to.K_SMALL, H, W), base, keys=("rgba", "depth_mm", "face_id"))
    mesh = _textured("cube", 41)
    poses = _poses(42, 3, 0.1, [1.3, 2.0, 3.5])
    a = _render(mesh, poses, K_OBJ, H, W)
    _same(_render(dict(mesh, faces=mesh["faces"][:, [0, 2, 1]], face_uv=mesh["face_uv"][:, [0, 2, 1]]), poses, K_OBJ, H, W), a)
    assert len(torch.unique(a["face_id"])) >= 6
    C = np.array([37, 200, 255], dtype=np.uint8)
    const = _render(dict(mesh, texture=np.full((16, 32, 3), C, np.uint8)), poses, K_OBJ, H, W)
    _same(const, _render({"vertices": mesh["vertices"], "faces": mesh["faces"], "colors": np.tile(C, (8, 1))}, poses, K_OBJ, H, W))


# ---- 4. the untextured path --------------------------------------------------------------------------------------------------------------
@gpu
def test_mesh_without_texture_renders_the_vertex_colour_entrys_bytes():
    m = ro.cube(0.4)
    mesh = {"vertices": m["vertices"], "faces": m["faces"], "colors": m["colors"], "uv": np.zeros((8, 2), np.float32)}     # UVs, no texture
    poses = _poses(52, 3, 0.1, [1.3, 2.0, 3.5])
    got = _render(mesh, poses, K_OBJ, H, W)
    L, V = _lib.lib(), len(poses)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (m["vertices"], m["faces"], m["colors"], poses.astype(np.float32))]
    per_view = (H * W + 12) * 8
    ws = torch.empty(256 + V * per_view, dtype=torch.uint8, device="cuda")
    out = {"rgba": torch.empty(V, H, W, 4, dtype=torch.uint8, device="cuda"), "depth_mm": torch.empty(V, H, W, dtype=torch.uint16, device="cuda"),
           "depth_m": torch.empty(V, H, W, dtype=torch.float32, device="cuda"), "face_id": torch.empty(V, H, W, dtype=torch.int32, device="cuda")}
    cnt = torch.empty(1, dtype=torch.int32, device="cuda")
    faces_h = np.ascontiguousarray(m["faces"])
    _lib.check(L.pp_render_views(dev[0].data_ptr(), 8, dev[1].data_ptr(), faces_h.ctypes.data, 12, dev[2].data_ptr(), dev[3].data_ptr(), V,
                                 60.0, 58.0, 31.5, 23.5, H, W, 1e-3, ws.data_ptr(), ws.numel(), out["rgba"].data_ptr(),
                                 out["depth_mm"].data_ptr(), out["depth_m"].data_ptr(), out["face_id"].data_ptr(), cnt.data_ptr(),
                                 _lib.stream_ptr()), "pp_render_views")
    _same(got, out)
    _same(got, ro.render(m["vertices"], m["faces"], m["colors"], poses.astype(np.float32), K_OBJ, H, W))
    assert (got["rgba"][..., 3] == 255).sum() > 500


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_textured_render_is_deterministic_across_runs_streams_and_chunks():
    mesh = _textured("icosphere", 61)
    poses = _poses(62, 4, 0.3, [1.0, 1.4, 2.0, 3.0])
    per_view = (H * W + len(mesh["faces"])) * 8
    base = _render(mesh, poses, K_OBJ, H, W)
    again = _render(mesh, poses, K_OBJ, H, W)
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        side = _render(mesh, poses, K_OBJ, H, W, workspace_bytes=256 + 3 * per_view)       # 2 chunks on a side stream
    one = _render(mesh, poses, K_OBJ, H, W, workspace_bytes=0)                             # 4 chunks
    torch.cuda.synchronize()
    for other in (again, side, one):
        _same(other, base)


# ---- 6. the bank ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_bank_of_a_textured_cube(golden_dir):
    views = np.load(os.path.join(golden_dir, "template_view_poses_level1.npy"))[::45]      # 4 views
    kw = {"K": np.array([[60.0, 0, 32.0], [0, 60.0, 24.0], [0, 0, 1.0]]), "resolution": (H, W), "units": "m", "img_size": 56, "pts_size": 16}
    mesh = _textured("cube", 71)
    C = np.array([180, 20, 99], dtype=np.uint8)
    coloured = tb.render_templates({"vertices": mesh["vertices"], "faces": mesh["faces"], "colors": np.tile(C, (8, 1))}, views, **kw)
    const = tb.render_templates(dict(mesh, texture=np.full((6, 12, 3), C, np.uint8), colors=np.zeros((8, 3), np.uint8)), views, **kw)
    assert set(const) == set(coloured) and coloured["tem_rgb"].shape == (4, 3, 56, 56)
    for k in coloured:
        assert torch.equal(const[k], coloured[k]), k              # the texture wins over "colors"
    rand = tb.render_templates(mesh, views, **kw)
    assert not torch.equal(rand["tem_rgb"], coloured["tem_rgb"]) and (rand["tem_rgb"] != coloured["tem_rgb"]).float().mean() > 0.1
    for k in ("tem_mask", "tem_pts3d", "tem_M", "tem_bbox", "tem_pose", "tem_K"):
        assert torch.equal(rand[k], coloured[k]), k


# ---- 7. argument validation ------------------------------------------------------------------------------------------------------------------
@gpu
def test_texture_entries_refuse_bad_arguments_before_any_launch():
    """The checks of tests/test_textured_bank_cpu.py with a device present: every call returns its error code from the host-side
    checks, nothing is enqueued, and the stream goes on working."""
    from test_textured_bank_cpu import test_texture_abi_argument_validation_needs_no_gpu as checks

    torch.cuda.synchronize()
    checks()
    torch.cuda.synchronize()
    assert int(torch.arange(5, device="cuda").sum().item()) == 10
