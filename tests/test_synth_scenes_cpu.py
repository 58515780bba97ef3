"""CPU: the numpy oracle of the scene composite (tests/synth_oracle.py) against hand-written answers; the lattice background; the pose
sampler; training_samples on a scene made without a GPU (render_oracle layers, the oracle composite); and every PP_EINVAL case of
pp_scene_composite and pp_depth_quantize_u16 through the C ABI with null or host pointers (validation comes before any device call)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_oracle as ro  # noqa: E402
import synth_oracle as so  # noqa: E402
from train_batch_oracle import hash3  # noqa: E402

from picopose_amd import _lib  # noqa: E402
from picopose_amd.provider import synth_scenes as ss  # noqa: E402
from picopose_amd.provider import training_batch as tb  # noqa: E402
from picopose_amd.provider.template_bank import mesh_diameter  # noqa: E402

F = np.float32


# ---- the oracle against answers written by hand ---------------------------------------------------------------------------------
def test_oracle_composite_by_hand():
    """2 x 3 frames.  Image 0 has layers 0, 1, 2: 0 and 1 tie at pixel (0, 1) (the lower index wins), 2 lies behind both wherever it
    covers (hidden).  Image 1 has no layer.  depth_scale 0.1 and 1.0."""
    H, W = 2, 3
    z = np.zeros((3, H, W), F)
    z[0] = [[0.5, 0.5, 0.0], [0.0, 0.0, 0.0]]
    z[1] = [[0.0, 0.5, 0.25], [0.0, 0.75, np.nan]]
    z[2] = [[0.0, 0.9, 0.9], [-1.0, 0.0, -0.0]]
    rgba = np.zeros((3, H, W, 4), np.uint8)
    for l in range(3):
        rgba[l, ..., :3] = (10 * (l + 1), 20 * (l + 1), 30 * (l + 1))        # alpha stays 0: it is never read
    desc = np.array([[0, 1 | 2 << 8 | 3 << 16, 0, 0], [0, 7 | 8 << 8 | 9 << 16, 0, 0]], np.int32)
    r = so.composite(rgba, z, [0, 3, 3], desc, [0.1, 1.0])
    assert r["instance"].tolist() == [[[0, 0, 1], [-1, 1, -1]], [[-1, -1, -1], [-1, -1, -1]]]
    assert r["depth"].tolist() == [[[5000, 5000, 2500], [0, 7500, 0]], [[0, 0, 0], [0, 0, 0]]]
    assert r["rgb"][0].tolist() == [[[10, 20, 30], [10, 20, 30], [20, 40, 60]], [[1, 2, 3], [20, 40, 60], [1, 2, 3]]]
    assert (r["rgb"][1] == np.array([7, 8, 9])).all()
    assert r["counts"].tolist() == [[2, 2], [3, 2], [2, 0]]
    assert r["boxes"].tolist() == [[0, 0, 1, 0], [1, 0, 2, 1], [0, 0, -1, -1]]
    assert r["mask_visib"].tolist() == [[[255, 255, 0], [0, 0, 0]], [[0, 0, 255], [0, 255, 0]], [[0, 0, 0], [0, 0, 0]]]


def test_oracle_depth_rounding_and_clamp():
    # 1000 Z / 0.1: half-way values round to even; beyond the 16-bit range the value clamps; +inf covers and clamps
    z = np.array([[[0.00025, 0.00035, 7.0, np.inf]]], F)
    rgba = np.zeros((1, 1, 4, 4), np.uint8)
    r = so.composite(rgba, z, [0, 1], np.zeros((1, 4), np.int32), [F(0.5)])
    q = np.rint((F(1000) * z[0, 0]) / F(0.5))
    assert r["depth"][0, 0].tolist() == [int(q[0]), int(q[1]), 14000, 65535]
    assert so.composite(rgba, z, [0, 1], np.zeros((1, 4), np.int32), [F(0.1)])["depth"][0, 0, 2] == 65535
    d = so.depth_quantize_u16(np.array([0.0, -1.0, np.nan, 0.12345, 0.00005, 0.00015, 7.0], F), 10000.0)
    assert d.tolist() == [0, 0, 0, int(np.rint(F(10000) * F(0.12345))), int(np.rint(F(10000) * F(0.00005))),
                          int(np.rint(F(10000) * F(0.00015))), 65535]


@pytest.mark.parametrize("s", [2, 5, 7])
def test_lattice_nodes_and_bounds(s):
    H, W, seed = 150, 200, 0x9ABCDEF1
    img = so.lattice(seed, s, H, W).astype(np.int64)
    S = 1 << s
    ys, xs = np.arange(0, H + S, S), np.arange(0, W + S, S)
    node = hash3(np.uint32(seed), (xs[None, :] // S).astype(np.uint32) * np.ones((len(ys), 1), np.uint32),
                 (ys[:, None] // S).astype(np.uint32) * np.ones((1, len(xs)), np.uint32)).astype(np.int64)
    col = np.stack([(node >> (8 * c)) & 255 for c in range(3)], -1)                 # (nodes_y, nodes_x, 3)
    ny, nx = (H - 1) // S + 1, (W - 1) // S + 1
    assert np.array_equal(img[::S, ::S], col[:ny, :nx])                             # at a node: the hashed colour
    gy, gx = np.mgrid[0:H, 0:W] // S
    four = np.stack([col[gy, gx], col[gy, gx + 1], col[gy + 1, gx], col[gy + 1, gx + 1]])
    assert (img >= four.min(0)).all() and (img <= four.max(0)).all()                # elsewhere: within the four nodes
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 50                          # and it is not flat


def test_background_modes():
    assert (so.background([0, 5 | 6 << 8 | 7 << 16, 0, 0], None, 2, 2) == np.array([5, 6, 7])).all()
    pic = np.arange(12, dtype=np.uint8).reshape(2, 2, 3)
    assert np.array_equal(so.background([1, 0, 0, 0], pic, 2, 2), pic)
    desc, images = ss.background_table([None, (1, 2, 3), pic, ("lattice", 0xFFFFFFFF, 3)], 4, 2, 2)
    assert desc.tolist() == [[0, 128 | 128 << 8 | 128 << 16, 0, 0], [0, 1 | 2 << 8 | 3 << 16, 0, 0], [1, 0, 0, 0], [2, -1, 3, 0]]
    assert np.array_equal(images[2], pic)
    assert np.array_equal(so.background(desc[3], None, 9, 9), so.lattice(0xFFFFFFFF, 3, 9, 9))
    for bad in [(1, 2, 300), ("lattice", 1, 8), ("lattice", 1, 1), ("noise", 1, 2), np.zeros((3, 2, 2, 3), np.uint8), [None]]:
        with pytest.raises(ValueError):
            ss.background_table(bad, 4, 2, 2)


# ---- the pose sampler -------------------------------------------------------------------------------------------------------------
K_FULL = np.array([[572.4114, 0, 320], [0, 573.57043, 240], [0, 0, 1.0]])


def test_sample_scene_poses_geometry_and_determinism():
    d = np.array([120.0, 277.0, 60.0])
    H, W, size, margin, near = 480, 640, (64.0, 200.0), 40.0, 1.0
    obj, img, poses = ss.sample_scene_poses(d, 50, (0, 4), K_FULL, (H, W), np.random.default_rng(5), size_px=size, margin_px=margin)
    U = len(obj)
    assert U > 50 and img.shape == (U,) and poses.shape == (U, 4, 4) and (np.diff(img) >= 0).all() and img.max() < 50
    assert set(obj.tolist()) == {0, 1, 2} and np.bincount(img, minlength=50).max() <= 4
    R, t = poses[:, :3, :3], poses[:, :3, 3]
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-12) and np.allclose(np.linalg.det(R), 1.0)
    u, v = K_FULL[0, 0] * t[:, 0] / t[:, 2] + K_FULL[0, 2], K_FULL[1, 1] * t[:, 1] / t[:, 2] + K_FULL[1, 2]
    eps = 1e-9
    assert (u >= margin - eps).all() and (u <= W - 1 - margin + eps).all() and (v >= margin - eps).all() and (v <= H - 1 - margin + eps).all()
    assert (t[:, 2] - d[obj] / 2 > near).all()
    s = 0.5 * (K_FULL[0, 0] + K_FULL[1, 1]) * d[obj] / t[:, 2]
    assert (s >= size[0] - eps).all() and (s <= size[1] + eps).all()
    again = ss.sample_scene_poses(d, 50, (0, 4), K_FULL, (H, W), np.random.default_rng(5), size_px=size, margin_px=margin)
    assert all(np.array_equal(a, b) for a, b in zip((obj, img, poses), again))
    other = ss.sample_scene_poses(d, 50, (0, 4), K_FULL, (H, W), np.random.default_rng(6), size_px=size, margin_px=margin)
    assert not (len(other[0]) == U and np.array_equal(other[2], poses))
    fixed = ss.sample_scene_poses(d, 7, 3, K_FULL, (H, W), np.random.default_rng(1))
    assert np.array_equal(fixed[1], np.repeat(np.arange(7), 3))
    # rotations are spread over the sphere: the mean rotated axis is near zero
    many = ss.sample_scene_poses(d, 400, 5, K_FULL, (H, W), np.random.default_rng(2))[2]
    assert np.abs(many[:, :3, 2].mean(0)).max() < 0.06


def test_sample_scene_poses_errors():
    rng = np.random.default_rng(0)
    ok = dict(diameters_mm=[100.0], n_images=2, per_image=1, K=K_FULL, resolution=(480, 640), generator=rng)
    ss.sample_scene_poses(**ok)
    for bad in (dict(size_px=(100.0, 1200.0)),           # f d / 1200 - d / 2 < 0: the front is behind the near plane
                dict(size_px=(100.0, 1140.0), near=1.0),  # ... within one millimetre of it
                dict(size_px=(0.0, 100.0)), dict(size_px=(200.0, 100.0)),
                dict(margin_px=240.0), dict(margin_px=-1.0), dict(diameters_mm=[0.0]), dict(diameters_mm=[]), dict(n_images=0),
                dict(per_image=(3, 2))):
        with pytest.raises(ValueError):
            ss.sample_scene_poses(**{**ok, **bad})


# ---- training_samples on a scene made on the CPU -------------------------------------------------------------------------------------
H_S, W_S = 60, 80
K_S = np.array([[70.0, 0, 39.5], [0, 70.0, 29.5], [0, 0, 1.0]])


def _euler(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    return (np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]) @
            np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]))


def _oracle_layers(mesh, poses_mm, K, H, W):
    """render_oracle works in metres, as the kernels do: millimetre vertices and translations scaled like render_views scales them."""
    v = (mesh["vertices"].astype(np.float64) * 1e-3).astype(F)
    p = np.array(poses_mm, dtype=np.float64)
    p[:, :3, 3] *= 1e-3
    return ro.render(v, mesh["faces"], mesh["colors"], p.astype(F), K, H, W)


@pytest.fixture(scope="module")
def cpu_scene(golden_dir):
    mesh = ro.cube(half=40.0)                                      # millimetres
    view_poses = np.load(os.path.join(golden_dir, "template_view_poses_level1.npy"))
    poses = np.tile(np.eye(4), (4, 1, 1))
    for k, (ang, t) in enumerate([((0.3, 0.4, 0.1), (-20.0, 0.0, 330.0)),          # 0: image 0, in front
                                  ((0.9, -0.2, 0.5), (-5.0, 5.0, 480.0)),          # 1: image 0, mostly behind instance 0
                                  ((-0.4, 0.8, 1.3), (30.0, -10.0, 300.0)),        # 2: image 1, alone
                                  ((0.1, 0.2, 0.3), (-450.0, -300.0, 1500.0))]):   # 3: image 1, far: a handful of pixels
        poses[k, :3, :3], poses[k, :3, 3] = _euler(*ang), t
    obj, img = np.zeros(4, np.int64), np.array([0, 0, 1, 1])
    lay = _oracle_layers(mesh, poses, K_S, H_S, W_S)
    assert lay["near_count"] == 0
    desc, _ = ss.background_table(("lattice", [3, 4], 3), 2, H_S, W_S)
    comp = so.composite(lay["rgba"], lay["depth_m"], [0, 2, 4], desc, [0.1, 0.1])
    c = comp["counts"].astype(np.float64)
    scene = {"rgb": comp["rgb"], "depth": comp["depth"], "instance_map": comp["instance"], "mask_visib": comp["mask_visib"],
             "px_count_all": comp["counts"][:, 0], "px_count_visib": comp["counts"][:, 1], "bbox_visib": comp["boxes"],
             "visib_fract": np.divide(c[:, 1], c[:, 0], out=np.zeros(4), where=c[:, 0] > 0)}
    renders = {}

    def render_frames(m, ids):
        rp, tem = ss.template_frame_poses(m, ids, view_poses)
        r = _oracle_layers(m, rp, K_S, H_S, W_S)
        for j, vid in enumerate(ids):
            renders[int(vid)] = r["depth_m"][j]
        return {"tem_rgba": r["rgba"], "tem_depth": so.depth_quantize_u16(r["depth_m"], 10000.0), "tem_pose": tem}

    return mesh, view_poses, poses, obj, img, scene, render_frames, renders


def test_training_samples_on_a_cpu_scene(cpu_scene):
    mesh, view_poses, poses, obj, img, scene, render_frames, renders = cpu_scene
    n_all, n_vis, fr = scene["px_count_all"], scene["px_count_visib"], scene["visib_fract"]
    print("px_count_all", n_all.tolist(), "px_count_visib", n_vis.tolist(), "visib_fract", fr.round(3).tolist())
    assert n_all[0] == n_vis[0] and 0 < fr[1] < 0.5 and n_all[1] >= 60 and fr[2] == 1.0 and 0 < n_all[3] < 40       # the scene is what the comments say
    kw = dict(min_visib_px=60, min_visib_fract=0.5, topk=5, render_frames=render_frames, return_index=True, template_K=K_S)
    samples, index = ss.training_samples(scene, poses, obj, img, [mesh], view_poses, K_S, np.random.default_rng(3), **kw)
    assert index["instance"].tolist() == [0, 2]                    # 1 fails the fraction, 3 the pixel count
    keys = {"rgb", "mask", "depth", "depth_scale", "K", "cam_R_m2c", "cam_t_m2c", "tem_rgba", "tem_depth", "tem_pose", "templates_K"}
    d_mm = mesh_diameter(mesh["vertices"])
    for s, u, view in zip(samples, index["instance"], index["view"]):
        assert set(s) == keys
        tb.check_sample(s)
        assert view in tb.nearest_template_views(poses[u, :3, :3], view_poses, 5)
        assert np.array_equal(s["rgb"], scene["rgb"][img[u]]) and np.array_equal(s["depth"], scene["depth"][img[u]])
        assert np.array_equal(s["mask"], scene["mask_visib"][u]) and s["depth_scale"] == 0.1
        assert np.array_equal(s["cam_R_m2c"].reshape(3, 3), poses[u, :3, :3]) and np.array_equal(s["cam_t_m2c"], poses[u, :3, 3])
        z = renders[int(view)]
        assert np.array_equal(s["tem_depth"], np.minimum(np.rint(F(10000) * z), 65535).astype(np.uint16)) and s["tem_depth"].max() > 0
        assert np.array_equal((s["tem_rgba"][..., 3] > 0), z > 0)
        # the unit rule of _prepare: t * 0.1 / 1000 is metres; the object sits at (0, 0, diameter)
        assert np.allclose(s["tem_pose"][:3, 3] * 0.1 / 1000.0, [0, 0, d_mm / 1000.0], rtol=0, atol=1e-12)
        assert np.array_equal(s["tem_pose"][:3, :3], view_poses[view, :3, :3])
        assert np.array_equal(s["templates_K"], K_S)
    # the real frame's units agree with its pose: the depth at the projected centre lies within the cube's extent of t_z
    for s in samples:
        t = s["cam_t_m2c"]
        u0, v0 = int(round(K_S[0, 0] * t[0] / t[2] + K_S[0, 2])), int(round(K_S[1, 1] * t[1] / t[2] + K_S[1, 2]))
        assert s["mask"][v0, u0] == 255 and abs(s["depth"][v0, u0] * s["depth_scale"] - t[2]) < 40 * np.sqrt(3)
    # thresholds: everything visible passes with none; the reference's defaults drop these small instances
    all_kept = ss.training_samples(scene, poses, obj, img, [mesh], view_poses, K_S, np.random.default_rng(3),
                                   **{**kw, "min_visib_px": 1, "min_visib_fract": 0.0})[1]["instance"]
    assert all_kept.tolist() == [0, 1, 2, 3]
    assert ss.training_samples(scene, poses, obj, img, [mesh], view_poses, K_S, np.random.default_rng(3), render_frames=render_frames, template_K=K_S) == []
    # the same Generator state draws the same views
    again = ss.training_samples(scene, poses, obj, img, [mesh], view_poses, K_S, np.random.default_rng(3), **kw)[1]
    assert np.array_equal(again["view"], index["view"])


# ---- the C ABI rejects bad arguments before any device call ----------------------------------------------------------------------
PP_EINVAL, PP_EWORKSPACE = -1, -2


def _composite_args(**over):
    """A valid argument set for 2 images of 4 x 8 with 3 layers, every `device` pointer a host buffer (never dereferenced: the
    tests below only make calls that fail validation)."""
    buf = (ctypes.c_char * 4096)()
    keep = [buf]
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    off = np.array([0, 2, 3], np.int32)
    desc = np.array([[0, 0, 0, 0], [2, 5, 3, 0]], np.int32)
    scale = np.array([0.1, 1.0], np.float32)
    a = dict(layers_rgba=p, layers_depth=p, layer_off=p, layer_off_host=off, n_layers=3, n_images=2, H=4, W=8, background=p,
             background_host=desc, bg_images=None, depth_scale=p, depth_scale_host=scale, workspace=p, workspace_bytes=2048, rgb=p,
             depth=p, instance=p, counts=p, boxes=p, mask_visib=None, stream=None)
    a.update(over)
    keep.extend(v for v in a.values() if isinstance(v, np.ndarray))
    return [v.ctypes.data if isinstance(v, np.ndarray) else v for v in a.values()], keep      # keep: what the pointers point into


def test_scene_composite_validation_needs_no_gpu():
    L = _lib.lib()

    def call(**kw):
        args, keep = _composite_args(**kw)
        rc = L.pp_scene_composite(*args)
        del keep
        return rc

    need = ctypes.c_size_t()
    assert L.pp_scene_composite_workspace_bytes(3, 4, 8, ctypes.byref(need)) == 0 and need.value == 256
    assert L.pp_scene_composite_workspace_bytes(5, 480, 640, ctypes.byref(need)) == 0 and need.value == (24 * 5 * 300 + 255) // 256 * 256
    assert L.pp_scene_composite_workspace_bytes(0, 4, 8, ctypes.byref(need)) == 0 and need.value == 0
    for bad in ((3, 4, 8, None), (-1, 4, 8, ctypes.byref(need)), (3, 0, 8, ctypes.byref(need)), (3, 4, -2, ctypes.byref(need)),
                (2048, 1024, 1024, ctypes.byref(need)), (1, 65536, 32768, ctypes.byref(need))):
        assert L.pp_scene_composite_workspace_bytes(*bad) == PP_EINVAL
    # a needed pointer that is null
    for name in ("layers_rgba", "layers_depth", "layer_off", "layer_off_host", "background", "background_host", "depth_scale",
                 "depth_scale_host", "rgb", "depth", "instance", "counts", "boxes"):
        assert call(**{name: None}) == PP_EINVAL, name
    # sizes
    for kw in (dict(n_images=0), dict(n_images=-1), dict(H=0), dict(W=0), dict(W=-8), dict(n_layers=-1),
               dict(H=32768, W=32768),                            # 3 layers of 2^30 samples
               dict(H=1024, W=1024, n_layers=2048, layer_off_host=np.array([0, 2, 2048], np.int32))):     # L H W = 2^31
        assert call(**kw) == PP_EINVAL, kw
    # the layer table
    for off in ([1, 2, 3], [0, 2, 2], [0, 2, 4], [0, 4, 3], [0, -1, 3]):
        assert call(layer_off_host=np.array(off, np.int32)) == PP_EINVAL, off
    # depth_scale
    for s in (0.0, -0.1, np.inf, np.nan):
        assert call(depth_scale_host=np.array([0.1, s], np.float32)) == PP_EINVAL, s
    # background descriptors
    for d in ([-1, 0, 0, 0], [3, 0, 0, 0], [2, 5, 1, 0], [2, 5, 8, 0], [1, 0, 0, 0]):
        assert call(background_host=np.array([[0, 0, 0, 0], d], np.int32)) == PP_EINVAL, d
    # the workspace
    args, keep = _composite_args()
    p = args[0]
    assert call(workspace=None) == PP_EWORKSPACE and call(workspace=p + 16) == PP_EWORKSPACE and call(workspace_bytes=255) == PP_EWORKSPACE


def test_depth_quantize_validation_needs_no_gpu():
    L = _lib.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    assert L.pp_depth_quantize_u16(None, 4, 10000.0, p, None) == PP_EINVAL
    assert L.pp_depth_quantize_u16(p, 4, 10000.0, None, None) == PP_EINVAL
    assert L.pp_depth_quantize_u16(p, -1, 10000.0, p, None) == PP_EINVAL
    for units in (0.0, -1.0, float("inf"), float("nan")):
        assert L.pp_depth_quantize_u16(p, 4, units, p, None) == PP_EINVAL
    assert L.pp_depth_quantize_u16(p, 0, 10000.0, p, None) == 0          # nothing to do: no launch
