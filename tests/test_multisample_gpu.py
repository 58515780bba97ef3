"""GPU: the multisampled render (pp_render_views_ms through render_views / render_templates / onboard_objects, samples=4) bit-equal
to tests/multisample_oracle.py for the three colour sources and the lit variants, its geometry outputs bit-equal to the
single-sample call, edge shapes, invariance under chunking / stream / view order, samples=1 unchanged, and the bank."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multisample_oracle as mo  # noqa: E402
import render_oracle as ro  # noqa: E402
from netcfg import small_cfg  # noqa: E402

from oracle.weights import seeded_state_dict  # noqa: E402
from picopose_amd import _lib  # noqa: E402
from picopose_amd.provider import template_bank as tb  # noqa: E402
from picopose_amd.utils.preprocess import _square  # noqa: E402

gpu = pytest.mark.gpu
GEOMETRY = ("depth_mm", "depth_m", "face_id")


def _render(mesh, poses, K, h, w, **kw):
    return tb.render_views(mesh, poses, K=K, resolution=(h, w), units="m", return_depth_m=True, return_face_id=True, check_near=False, **kw)


def _same(got, want, keys):
    for k in keys:
        a, b = got[k].cpu(), torch.from_numpy(want[k]) if isinstance(want[k], np.ndarray) else want[k].cpu()
        assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), k


@functools.lru_cache(maxsize=None)
def _scene(name):
    """A scene of the oracle module and its oracle render, computed once."""
    mesh, poses, K, (h, w), shading = mo.scenes()[name]
    want = mo.render(mesh, poses, K, h, w, mo.oracle_shading(shading, mesh))
    for v in range(len(poses)):                                  # (tests/test_multisample_cpu.py asserts the same without a GPU)
        stats = mo.edge_stats({k: want[k][v] for k in ("rgba", "face_id")})
        assert stats[0] >= 30 and min(stats[1:]) >= 10, (name, v, stats)
    return mesh, poses, K, h, w, shading, want


def _against_oracle(name):
    mesh, poses, K, h, w, shading, want = _scene(name)
    got = _render(mesh, poses, K, h, w, shading=shading, samples=4)
    one = _render(mesh, poses, K, h, w, shading=shading, samples=1)
    _same(got, want, ("rgba",) + GEOMETRY)
    _same(got, one, GEOMETRY)                                    # M5: the single-sample call's bytes
    assert int(got["near_count"].item()) == int(one["near_count"].item()) == want["near_count"] == 0
    _same(one, {"rgba": want["centre_rgba"]}, ("rgba",))
    assert not torch.equal(got["rgba"], one["rgba"])


@gpu
@pytest.mark.parametrize("name", ["cube", "icosphere"])
def test_vertex_colours_equal_the_oracle_and_geometry_the_single_sample_call(name):
    _against_oracle(name)


@gpu
@pytest.mark.parametrize("name", ["textured", "tless", "smooth_tone"])
def test_textured_and_lit_equal_the_oracle(name):
    _against_oracle(name)


@gpu
def test_edge_shapes_in_one_call():
    """One render call of mo.edge_scene(): sub-pixel triangles, a mesh off every side, a triangle at the near plane, and a second
    view with partial pixels only, on which pp_template_extents gives the oracle's box.  render_templates places its object itself
    (t = (0, 0, diameter)), so it cannot be given this frame: the bank of a partial-pixels-only view is the next test, on a frame
    of its own."""
    mesh, poses, K, (h, w) = mo.edge_scene()
    want = mo.render(mesh, poses, K, h, w)
    got = _render(mesh, poses, K, h, w, samples=4)
    _same(got, want, ("rgba",) + GEOMETRY)
    assert int(got["near_count"].item()) == want["near_count"] == 1            # once, not once per plane
    assert int(_render(mesh, poses, K, h, w)["near_count"].item()) == 1
    far = got["rgba"][1, ..., 3]
    assert int(far.max()) < 255 and int((far > 0).sum()) >= 1                 # partial pixels only
    ext = torch.empty(2, 4, dtype=torch.int32, device="cuda")
    cnt = torch.empty(2, dtype=torch.int32, device="cuda")
    _lib.call("pp_template_extents", got["rgba"], 2, h, w, ext, cnt)
    for v in range(2):
        ys, xs = np.nonzero(want["rgba"][v, ..., 3])
        assert ext[v].tolist() == [int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())] and int(cnt[v]) == len(ys)


@gpu
def test_bank_of_another_frame_with_partial_pixels_only():
    """Not the frame of test_edge_shapes_in_one_call: mo.speck_scene(), which render_templates can place itself.  A speck that
    covers one sample of each of four pixels: the multisampled bank has a box and, with no alpha of 255, an empty
    mask, where the single-sample bank of the same call has a full one."""
    mesh, views, K, (h, w) = mo.speck_scene()
    poses = tb.template_object_poses(views, mesh["vertices"])
    want = mo.render(mesh, poses.astype(np.float32), K, h, w)
    assert want["rgba"][0, ..., 3].max() == 64 and (want["rgba"][0, ..., 3] > 0).sum() == 4 and np.all(want["rgba"][0, 24:26, 32:34, 3] == 64)
    frames = _render(mesh, poses, K, h, w, samples=4)
    _same(frames, want, ("rgba",) + GEOMETRY)
    kw = {"K": K, "resolution": (h, w), "units": "m", "img_size": 28, "pts_size": 16}
    bank = tb.render_templates(mesh, views, samples=4, **kw)
    assert bank["tem_bbox"][0].tolist() == [24.0, 26.0, 32.0, 34.0]
    assert float(bank["tem_mask"].abs().max()) == 0.0 and bool(torch.isfinite(bank["tem_rgb"]).all())
    one = tb.render_templates(mesh, views, **kw)
    assert one["tem_bbox"][0].tolist() == [24.0, 26.0, 32.0, 34.0] and float(one["tem_mask"].min()) == 1.0
    assert torch.equal(bank["tem_pts3d"], one["tem_pts3d"])                   # the centres are hit: same depth, same points


@gpu
def test_chunking_stream_and_view_order_do_not_change_the_bytes():
    mesh, poses, K, h, w, _, want = _scene("icosphere")
    keys = ("rgba",) + GEOMETRY
    one_view = _lib.workspace_bytes("pp_render_ms_workspace_bytes", h, w, len(mesh["faces"]), 1, 4)
    all_views = _lib.workspace_bytes("pp_render_ms_workspace_bytes", h, w, len(mesh["faces"]), len(poses), 4)
    assert one_view - 256 == 5 * (h * w + len(mesh["faces"])) * 8 and all_views - 256 == len(poses) * (one_view - 256)
    base = _render(mesh, poses, K, h, w, samples=4, workspace_bytes=all_views)
    chunked = _render(mesh, poses, K, h, w, samples=4, workspace_bytes=one_view)              # a chunk per view
    short = _render(mesh, poses, K, h, w, samples=4, workspace_bytes=0)                       # at least one view's worth is allocated
    side_stream = torch.cuda.Stream()
    side_stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side_stream):
        side = _render(mesh, poses, K, h, w, samples=4, workspace_bytes=2 * one_view)
    torch.cuda.synchronize()
    back = _render(mesh, poses[::-1].copy(), K, h, w, samples=4)
    _same(base, want, keys)
    for other in (chunked, short, side):
        _same(other, base, keys)
    _same({k: back[k].flip(0) for k in keys}, base, keys)


def _entry_ms(mesh, poses, K, h, w, samples):
    """pp_render_views_ms called directly for a vertex-coloured mesh in metres (unlit)."""
    v, f, c = (np.ascontiguousarray(mesh[k]) for k in ("vertices", "faces", "colors"))
    V = len(poses)
    v_d, f_d, c_d, p_d = (torch.from_numpy(a).cuda() for a in (v, f, c, np.ascontiguousarray(poses, dtype=np.float32)))
    ws = torch.empty(_lib.workspace_bytes("pp_render_ms_workspace_bytes", h, w, len(f), V, samples), dtype=torch.uint8, device="cuda")
    out = {"rgba": torch.empty(V, h, w, 4, dtype=torch.uint8, device="cuda"), "depth_mm": torch.empty(V, h, w, dtype=torch.uint16, device="cuda"),
           "depth_m": torch.empty(V, h, w, dtype=torch.float32, device="cuda"), "face_id": torch.empty(V, h, w, dtype=torch.int32, device="cuda"),
           "near_count": torch.empty(1, dtype=torch.int32, device="cuda")}
    _lib.call("pp_render_views_ms", v_d, len(v), f_d, f, len(f), c_d, None, None, 0, 0, p_d, V, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
              float(K[1, 2]), h, w, 1e-3, ws, ws.numel(), out["rgba"], out["depth_mm"], out["depth_m"], out["face_id"], out["near_count"],
              0, None, 0, 0.0, 0, None, None, None, 0, samples)
    return out


@gpu
def test_samples_1_is_the_default_render_through_either_entry():
    keys = ("rgba",) + GEOMETRY + ("near_count",)
    for name in ("cube", "textured", "tless"):
        mesh, poses, K, h, w, shading, want = _scene(name)
        _same(_render(mesh, poses, K, h, w, shading=shading, samples=1), _render(mesh, poses, K, h, w, shading=shading), keys)
    mesh, poses, K, h, w, _, want = _scene("cube")
    default = _render(mesh, poses, K, h, w)
    _same(_entry_ms(mesh, poses, K, h, w, 1), default, keys)
    _same(_entry_ms(mesh, poses, K, h, w, 4), want, ("rgba",) + GEOMETRY)


def _views(golden_dir):
    return np.load(os.path.join(golden_dir, "template_view_poses_level1.npy"))[::45]          # 4 views


@gpu
def test_multisampled_frames_reach_the_bank(golden_dir):
    mesh, K, (h, w) = mo.bank_scene()
    views = _views(golden_dir)
    poses = tb.template_object_poses(views, mesh["vertices"])
    want = mo.render(mesh, poses.astype(np.float32), K, h, w)
    def window(mask):
        ys, xs = np.nonzero(mask)
        return _square(int(ys.min()), int(ys.max()) + 1, int(xs.min()), int(xs.max()) + 1, h, w)

    grown = [v for v in range(4) if window(want["rgba"][v, ..., 3] > 0) != window(want["face_id"][v] >= 0)]
    assert 0 < len(grown) < 4                                                 # the oracle: some windows grow with alpha > 0, some do not
    kw = {"K": K, "resolution": (h, w), "units": "m", "img_size": 28, "pts_size": 16}
    ms = tb.render_templates(mesh, views, samples=4, **kw)
    one = tb.render_templates(mesh, views, **kw)
    frames = tb.render_views(mesh, poses, K=K, resolution=(h, w), units="m", samples=4)
    _same(frames, want, ("rgba", "depth_mm"))
    poses_file = poses.copy()
    poses_file[:, :3, 3] *= 1.0 / 1000.0                                       # render_templates' own factor for units="m" (tem_pose is t / 1000 again)
    again = tb.templates_from_frames(frames["rgba"], frames["depth_mm"], K, poses_file, img_size=28, pts_size=16)
    assert set(ms) == set(again) == set(one)
    for k in ms:
        assert ms[k].dtype == again[k].dtype and torch.equal(ms[k], again[k]), k
    assert torch.equal(ms["tem_pose"], one["tem_pose"]) and torch.equal(ms["tem_K"], one["tem_K"])
    agree = (ms["tem_bbox"] == one["tem_bbox"]).all(dim=1)
    assert torch.equal(ms["tem_pts3d"][agree], one["tem_pts3d"][agree])
    assert [v for v in range(4) if not bool(agree[v])] == grown
    for v in grown:                                                           # a grown window is no smaller
        b4, b1 = ms["tem_bbox"][v].tolist(), one["tem_bbox"][v].tolist()
        assert b4[1] - b4[0] >= b1[1] - b1[0] and b4 == [float(x) for x in window(want["rgba"][v, ..., 3] > 0)]
    assert not torch.equal(ms["tem_rgb"], one["tem_rgb"])


@gpu
def test_onboard_objects_forwards_samples(golden_dir, monkeypatch):
    from picopose_amd import ops
    from picopose_amd.picopose import Net

    monkeypatch.setattr(ops, "SATURATION_FLAG", False)       # (plain seeded weights leave the f16x3 range: test_e2e.py explains)
    net = Net(small_cfg())
    net.load_state_dict(seeded_state_dict(net.state_dict(), 5))
    net = net.cuda().eval()
    meshes = [ro.cube(40.0), ro.icosphere(3, 50.0)]
    views = _views(golden_dir)
    one = tb.onboard_objects(net, meshes, views, bs=3)
    ms = tb.onboard_objects(net, meshes, views, bs=3, samples=4)
    assert set(ms) == set(one)
    for k in one:
        assert ms[k].dtype == one[k].dtype and ms[k].shape == one[k].shape, k
    assert bool(torch.isfinite(ms["template_feature"]).all()) and not torch.equal(ms["tem_rgb"], one["tem_rgb"])
