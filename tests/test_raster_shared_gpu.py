"""GPU: the two rasterisers are one.  The template renderer (pp_render_views, whole frames) and the windowed depth raster
(pp_vsd_errors, through evaluation.render_depth) render the same float32 mesh, pose, camera and near plane to the same depth BITS: on
a 45 x 61 frame (odd, no multiple of the 16-sample tile), for triangles that take the queue and tile path (a cube) and for triangles a
single lane walks (an icosphere of 1 280 faces), centred, cut by the right and bottom frame edges, and smaller than a sample."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_oracle as ro  # noqa: E402

from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd.provider import template_bank as tb  # noqa: E402

H, W, NEAR = 45, 61, 1.0
K = np.array([[100.0, 0, 30.5], [0, 100.0, 22.5], [0, 0, 1.0]])
MESHES = {"cube": lambda: ro.cube(40.0), "icosphere": lambda: ro.icosphere(3, 50.0)}
# centred; cut by the right and bottom frame edges; so far away that the whole object is about a sample wide
T = np.array([[0, 0, 400.0], [110, 80, 400.0], [-945, -585, 9000.0]])


def _poses():
    rng = np.random.default_rng(8)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3, 3)))
    P = np.tile(np.eye(4), (3, 1, 1))
    P[:, :3, :3] = q * np.sign(np.linalg.det(q))[:, None, None]
    P[:, :3, 3] = T
    return P.astype(np.float32)


def _both(name, window):
    """-> the mesh, the poses, render_views' depth and render_depth's (3, H, W) float32, on the host."""
    mesh, P = MESHES[name](), _poses()
    frames = tb.render_views(mesh, P, K=K, resolution=(H, W), units="m", near=NEAR, return_depth_m=True)   # "m": the arrays as they are
    models = ev.ObjectModels({1: {"vertices": mesh["vertices"], "faces": mesh["faces"], "info": {"diameter": 140.0}}})
    depth = ev.render_depth(models, [1, 1, 1], P[:, :3, :3], P[:, :3, 3], K, (H, W), near=NEAR, window=window)
    assert int(frames["near_count"].item()) == 0 and depth["near_count"] == 0
    return mesh, P, frames["depth_m"].cpu().numpy(), depth["depth"].cpu().numpy(), models


def _boxes(mesh, pose):
    """the sample boxes of the view's triangles that can cover a sample, and the faces that do cover one"""
    tri = ro.Triangles(mesh["vertices"], mesh["faces"], pose, (100.0, 100.0, 30.5, 22.5), H, W, NEAR)
    size = ((tri.bx1 - tri.bx0 + 1) * (tri.by1 - tri.by0 + 1))[tri.keep]
    covering = np.unique(np.concatenate([face for _, face, _ in tri.fragments(H, W)] + [np.zeros(0, dtype=np.int64)]))
    return size, covering


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube", "icosphere"])
def test_whole_frame_depth_of_the_two_rasterisers_is_the_same_bits(name):
    mesh, P, a, b, _ = _both(name, "full")
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (3, H, W)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # the views are what the docstring says they are
    size, covering = _boxes(mesh, P[0])
    if name == "cube":
        assert len(size) == 12 and size.min() > 64                           # every triangle goes through the queue, over several tiles
    else:
        assert len(mesh["faces"]) == 1280 and size.max() <= 64              # every triangle is walked by its lane
    cover = a > 0
    assert cover[0].sum() > 400 and not (cover[0][0].any() or cover[0][-1].any() or cover[0][:, 0].any() or cover[0][:, -1].any())
    assert cover[1][-1].any() and cover[1][:, -1].any() and not cover[1][0].any()
    _, far = _boxes(mesh, P[2])
    assert cover[2].any() and len(far) < len(mesh["faces"]) / 2             # most triangles cover no sample


@pytest.mark.gpu
def test_windowed_cube_depth_equals_the_frame_inside_the_window_and_is_background_outside():
    mesh, P, a, b, models = _both("cube", "auto")
    for v in range(3):
        x0, y0, x1, y1 = ev.plan_window(models.aabb_corners[0], P[v], (100.0, 100.0, 30.5, 22.5), H, W, NEAR)
        assert 0 < (x1 - x0) * (y1 - y0) < H * W
        inside = np.zeros((H, W), dtype=bool)
        inside[y0:y1, x0:x1] = True
        assert np.array_equal(a[v][inside].view(np.int32), b[v][inside].view(np.int32)) and (a[v][inside] > 0).any()
        assert not b[v][~inside].any() and not a[v][~inside].any()
