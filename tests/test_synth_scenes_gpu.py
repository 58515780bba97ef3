"""GPU: the scene composite (csrc/pp_synth.hip via picopose_amd/provider/synth_scenes.py) bit for bit against the numpy oracle
(tests/synth_oracle.py) on synthetic and on rendered layers; determinism over streams, call splits and image order; the units of a
training sample closed geometrically on a sphere; and meshes -> training_samples -> assemble_training_batch -> a training step."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_oracle as ro  # noqa: E402
import synth_oracle as so  # noqa: E402

from picopose_amd.provider import synth_scenes as ss  # noqa: E402
from picopose_amd.provider import training_batch as tb  # noqa: E402
from picopose_amd.provider.template_bank import TEMPLATE_K, render_views  # noqa: E402

gpu = pytest.mark.gpu
F = np.float32
U32 = 2.0 ** -24                                                # float32 unit roundoff


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _random_layers(rng, counts, H, W):
    """Layers with few distinct depths (exact ties) and, in an image of 9 layers: a fully hidden layer (3, behind 1), a layer that
    covers nothing (5), NaN / negative / -0.0 samples (6), two layers nearer than the rest (7, 8), a depth that clamps at 65535
    units where nothing else covers, and pixels that stay background."""
    L = int(sum(counts))
    levels = np.array([0.0, 0.0, 0.25, 0.4000001, 0.4000001, 0.75, 1.5], F)
    z = levels[rng.integers(0, len(levels), (L, H, W))]
    rgba = rng.integers(0, 256, (L, H, W, 4)).astype(np.uint8)
    l0 = 0
    for n in counts:
        if n >= 9:
            z[l0 + 5] = rng.choice(np.array([0.0, -0.0, -1.0, np.nan], F), (H, W))
            bad = rng.random((H, W)) < 0.2
            z[l0 + 6][bad] = rng.choice(np.array([-0.0, -2.5, np.nan], F), int(bad.sum()))
            z[l0 + 7][rng.random((H, W)) < 0.1] = F(0.2)
            z[l0 + 8][rng.random((H, W)) < 0.1] = F(0.1)
            if W >= 5:
                z[l0:l0 + 9, 0, :5] = 0                                       # columns 3, 4 of row 0: background
                z[l0 + 2, 0, :3] = F(7.0)                                     # 70000 units at depth_scale 0.1: clamps
            z[l0 + 3] = np.where(z[l0 + 1] > 0, z[l0 + 1] + F(1.0), 0)        # behind layer 1 wherever it covers: hidden
        l0 += n
    return rgba, z


def _modes(rng, n, H, W):
    """The three background modes in turn over the images, two depth scales."""
    pics = rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    bgs = [("lattice", 0xDEADBEEF + i, 2 + i % 6) if i % 3 == 0 else (pics[i] if i % 3 == 1 else (9, 200, 77)) for i in range(n)]
    return bgs, np.array([0.1, 1.0, 0.1][:n], F)


def _assert_equal(got, ref, masks=True):
    for a, b in (("rgb", "rgb"), ("depth", "depth"), ("instance_map", "instance"), ("bbox_visib", "boxes")):
        assert np.array_equal(_np(got[a]), ref[b]), a
    assert np.array_equal(_np(got["px_count_all"]), ref["counts"][:, 0]) and np.array_equal(_np(got["px_count_visib"]), ref["counts"][:, 1])
    if masks:
        assert np.array_equal(_np(got["mask_visib"]), ref["mask_visib"])
    else:
        assert "mask_visib" not in got


@gpu
@pytest.mark.parametrize("counts", [[9], [0], [1, 0, 9]])
@pytest.mark.parametrize("H,W", [(37, 53), (8, 64), (1, 1)])
def test_composite_kernel_equals_the_oracle(H, W, counts):
    """37 x 53: W no multiple of 4 (one pixel per access), H W no multiple of the workgroup's 1024 pixels, two workgroups per image;
    8 x 64: the four-pixels-per-lane path; 1 x 1.  0, 1 and 9 layers in an image; L = 0 as a whole call."""
    rng = np.random.default_rng(H * 1000 + W + len(counts))
    n = len(counts)
    rgba, z = _random_layers(rng, counts, H, W)
    layer_image = np.repeat(np.arange(n), counts)
    bgs, scales = _modes(rng, n, H, W)
    desc, pics = ss.background_table(bgs, n, H, W)
    ref = so.composite(rgba, z, np.concatenate([[0], np.cumsum(counts)]), desc, scales, pics)
    got = ss.composite_layers(rgba, z, layer_image, n, backgrounds=bgs, depth_scale=scales)
    _assert_equal(got, ref)
    fr = ref["counts"].astype(np.float64)
    assert np.array_equal(got["visib_fract"], np.divide(fr[:, 1], fr[:, 0], out=np.zeros(len(fr)), where=fr[:, 0] > 0))
    _assert_equal(ss.composite_layers(rgba, z, layer_image, n, backgrounds=bgs, depth_scale=scales, masks=False), ref, masks=False)
    if max(counts) >= 9 and H * W > 1:                              # the content is what the docstring of _random_layers says
        l0 = int(np.cumsum(counts)[-1]) - 9
        assert ref["counts"][l0 + 3, 0] > 0 and ref["counts"][l0 + 3, 1] == 0 and ref["counts"][l0 + 5, 0] == 0
        assert (ref["depth"] == 65535).any() and (ref["instance"] == -1).any()
        assert ref["boxes"][l0 + 5].tolist() == [0, 0, -1, -1]


@gpu
def test_composite_layers_scatters_back_to_the_callers_order():
    """Layers given in any image order: per-layer results come back in the caller's order and instance_map holds the caller's indices."""
    rng = np.random.default_rng(4)
    H, W, counts = 12, 20, [2, 3, 1]
    rgba, z = _random_layers(rng, counts, H, W)
    layer_image = np.repeat(np.arange(3), counts)
    ref = so.composite(rgba, z, [0, 2, 5, 6], np.tile(np.array([0, 128 | 128 << 8 | 128 << 16, 0, 0], np.int32), (3, 1)), [F(0.1)] * 3)
    perm = np.array([2, 0, 5, 3, 1, 4])                            # caller's layer k is sorted layer perm[k]; an image's layers keep their order
    got = ss.composite_layers(rgba[perm], z[perm], layer_image[perm], 3)
    assert np.array_equal(_np(got["rgb"]), ref["rgb"]) and np.array_equal(_np(got["depth"]), ref["depth"])
    assert np.array_equal(_np(got["px_count_visib"]), ref["counts"][perm, 1]) and np.array_equal(_np(got["bbox_visib"]), ref["boxes"][perm])
    assert np.array_equal(_np(got["mask_visib"]), ref["mask_visib"][perm])
    inv = np.argsort(perm)
    assert np.array_equal(_np(got["instance_map"]), np.where(ref["instance"] >= 0, inv[np.maximum(ref["instance"], 0)], -1))


@gpu
@pytest.mark.parametrize("n,offset", [(1, 0), (7, 0), (4096 + 3, 0), (1030, 1)])
def test_depth_quantizer_equals_the_oracle(n, offset):
    rng = np.random.default_rng(n)
    z = rng.choice(np.array([0.0, -0.0, -1.0, np.nan, 0.00005, 0.00015, 0.00025, 0.12345, 0.5, 6.5535, 6.55355, 7.0, np.inf], F), n + offset)
    zr = np.where(rng.random(n + offset) < 0.5, rng.random(n + offset).astype(F) * F(3), z).astype(F)
    d = torch.from_numpy(zr).cuda()[offset:]                       # offset 1: a buffer that is not 16-byte aligned
    assert np.array_equal(_np(ss.depth_quantize_u16(d, 10000.0)), so.depth_quantize_u16(zr[offset:], 10000.0))
    assert np.array_equal(_np(ss.depth_quantize_u16(d, 1000.0)), so.depth_quantize_u16(zr[offset:], 1000.0))


# ---- rendered layers ----------------------------------------------------------------------------------------------------------------
H_S, W_S = 48, 64
K_S = np.array([[70.0, 0, 31.5], [0, 70.0, 23.5], [0, 0, 1.0]])


def _euler(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    return (np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]) @
            np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]))


def _pose(ang, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = _euler(*ang), t
    return P


def _small_scene():
    """The cube (two large triangles per face) and icosphere(2), the sphere shaded.  Image 0: cube in front of a sphere and a second
    cube behind both; image 1: one unoccluded sphere; image 2: a cube cut by the frame border and a sphere."""
    meshes = [ro.cube(half=40.0), ro.icosphere(2, 45.0)]
    inst = [(0, 0, (0.3, 0.4, 0.1), (-15.0, 0.0, 330.0)), (1, 0, (0.0, 0.0, 0.0), (10.0, 5.0, 420.0)),
            (0, 0, (0.9, -0.2, 0.5), (0.0, 0.0, 600.0)), (1, 1, (0.5, 0.1, 0.2), (-20.0, 10.0, 380.0)),
            (0, 2, (-0.4, 0.8, 1.3), (150.0, -10.0, 400.0)), (1, 2, (0.2, 0.2, 0.2), (-40.0, 20.0, 500.0))]
    obj = np.array([m for m, *_ in inst])
    img = np.array([i for _, i, *_ in inst])
    poses = np.stack([_pose(a, t) for *_, a, t in inst])
    return meshes, obj, img, poses, [None, "tless"]


@gpu
def test_render_scenes_equals_the_oracle_on_rendered_layers():
    meshes, obj, img, poses, shading = _small_scene()
    bgs = [("lattice", 11, 3), (30, 60, 90), ("lattice", 12, 4)]
    scene = ss.render_scenes(meshes, obj, img, poses, K_S, (H_S, W_S), backgrounds=bgs, shading=shading, depth_scale=[0.1, 1.0, 0.1])
    rgba = np.zeros((len(obj), H_S, W_S, 4), np.uint8)
    z = np.zeros((len(obj), H_S, W_S), F)
    for m in (0, 1):                                               # the layers, as render_scenes asks render_views for them
        r = render_views(meshes[m], poses[obj == m], K=K_S, resolution=(H_S, W_S), return_depth_m=True, shading=shading[m])
        rgba[obj == m], z[obj == m] = _np(r["rgba"]), _np(r["depth_m"])
    desc, _ = ss.background_table(bgs, 3, H_S, W_S)
    ref = so.composite(rgba, z, [0, 3, 4, 6], desc, np.array([0.1, 1.0, 0.1], F))
    _assert_equal(scene, ref)
    assert scene["n_groups"] == 1
    n_all, n_vis = ref["counts"].T
    print("px_count_all", n_all.tolist(), "px_count_visib", n_vis.tolist())
    assert n_all[0] == n_vis[0] > 300 and 0 < n_vis[1] < n_all[1] and n_vis[2] < n_all[2] and n_all.min() > 50
    # the image with one unoccluded instance is that render_views frame over its background, and its visible mask is the alpha
    alpha = rgba[3, ..., 3] > 0
    assert np.array_equal(_np(scene["mask_visib"])[3], np.where(alpha, 255, 0)) and alpha.sum() == n_all[3] == n_vis[3]
    frame = np.where(alpha[..., None], rgba[3, ..., :3], np.array([30, 60, 90], np.uint8))
    assert np.array_equal(_np(scene["rgb"])[1], frame)
    assert np.array_equal(_np(scene["depth"])[1], np.where(alpha, np.rint(F(1000) * z[3]), 0).astype(np.uint16))      # depth_scale 1
    assert np.array_equal(scene["visib_fract"], n_vis / n_all)
    # a triangle at the near plane raises, as render_templates does
    close = poses.copy()
    close[0, 2, 3] = 30.0
    with pytest.raises(ValueError, match="near plane"):
        ss.render_scenes(meshes, obj, img, close, K_S, (H_S, W_S))


@gpu
def test_render_scenes_is_deterministic():
    """The same bits on another stream, with a workspace bound that forces several composite calls, and under a permutation of the
    images (with the instances reordered too: instance_map then holds the permuted indices)."""
    meshes, obj, img, poses, shading = _small_scene()
    seeds = np.array([11, 12, 13])
    kw = dict(shading=shading, depth_scale=0.1)
    base = ss.render_scenes(meshes, obj, img, poses, K_S, (H_S, W_S), backgrounds=("lattice", seeds, 3), **kw)
    keys = ("rgb", "depth", "instance_map", "px_count_all", "px_count_visib", "bbox_visib", "mask_visib")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ss.render_scenes(meshes, obj, img, poses, K_S, (H_S, W_S), backgrounds=("lattice", seeds, 3), **kw)
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(base[k], other[k]), k
    per_layer = H_S * W_S * 9 + 24 * ((H_S * W_S + 1023) // 1024)
    split = ss.render_scenes(meshes, obj, img, poses, K_S, (H_S, W_S), backgrounds=("lattice", seeds, 3), workspace_bytes=3 * per_layer, **kw)
    assert split["n_groups"] == 2
    for k in keys:
        assert torch.equal(base[k], split[k]), k
    with pytest.raises(ValueError, match="workspace_bytes"):
        ss.render_scenes(meshes, obj, img, poses, K_S, (H_S, W_S), workspace_bytes=2 * per_layer, **kw)
    image_perm = np.array([2, 0, 1])                               # image i becomes image image_perm[i]
    order = np.array([4, 3, 0, 5, 1, 2])                           # new instance k is old instance order[k]; per image the order is kept
    moved = ss.render_scenes(meshes, obj[order], image_perm[img[order]], poses[order], K_S, (H_S, W_S),
                             backgrounds=("lattice", seeds[np.argsort(image_perm)], 3), **kw)
    for k in ("rgb", "depth"):
        assert np.array_equal(_np(base[k]), _np(moved[k])[image_perm]), k
    for k in ("px_count_all", "px_count_visib", "bbox_visib", "mask_visib"):
        assert np.array_equal(_np(base[k])[order], _np(moved[k])), k
    old = _np(moved["instance_map"])[image_perm]
    assert np.array_equal(np.where(old >= 0, order[np.maximum(old, 0)], -1), _np(base["instance_map"]))


@gpu
def test_sample_geometry_closes_on_a_sphere():
    """An icosphere(3) of radius R (mm) at a drawn pose: the sample's depth at its mask pixels, back-projected with the sample's K and
    taken into the object frame with the sample's pose, lies between the mesh's inscribed sphere and R.  The mesh is inscribed in the
    sphere of radius R and contains the ball of radius r_in = the least distance of a face plane from the centre, so every surface
    point has r_in <= |X| <= R.  Allowances, all in millimetres: the raster's (test_oracle_icosphere_depth_between_sphere_and_sag: the
    1/256 px snap and the projection's roundings, (1 / 512 + 3 u W) Z / f sideways, plus 11 u Z); half a depth unit along the ray,
    0.5 depth_scale |d| with d = ((x - cx) / fx, (y - cy) / fy, 1), plus the two float32 roundings of the quantiser, 2 u of the
    value; and the float32 roundings of the vertices and the translation on the way to metres, 2 u (R + |t|)."""
    R0, H, W = 50.0, 240, 320
    K = np.array([[286.2, 0, 160.0], [0, 286.8, 120.0], [0, 0, 1.0]])
    mesh = ro.icosphere(3, R0)
    tri = mesh["vertices"].astype(np.float64)[mesh["faces"]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    r_in = np.abs(np.einsum("ij,ij->i", nrm / np.linalg.norm(nrm, axis=1, keepdims=True), tri[:, 0])).min()
    assert 0.98 * R0 < r_in < R0
    rng = np.random.default_rng(8)
    obj, img, poses = ss.sample_scene_poses([2 * R0], 2, 1, K, (H, W), rng, size_px=(60.0, 120.0), margin_px=70.0)
    for depth_scale in (0.1, 1.0):
        scene = ss.render_scenes([mesh], obj, img, poses, K, (H, W), depth_scale=depth_scale)
        samples = ss.training_samples(scene, poses, obj, img, [mesh], np.tile(np.eye(4), (3, 1, 1)), K, rng, min_visib_px=100,
                                      depth_scale=depth_scale, render_frames=lambda m, ids: {
                                          "tem_rgba": np.zeros((len(ids), 2, 2, 4), np.uint8), "tem_depth": np.zeros((len(ids), 2, 2), np.uint16),
                                          "tem_pose": np.tile(np.eye(4), (len(ids), 1, 1))})
        assert len(samples) == 2
        for s in samples:
            Rm, t, Ks = s["cam_R_m2c"].reshape(3, 3), s["cam_t_m2c"], s["K"]
            yy, xx = np.nonzero(s["mask"])
            assert len(yy) > 2000
            Z = s["depth"][yy, xx].astype(np.float64) * s["depth_scale"]              # millimetres
            d = np.stack([(xx - Ks[0, 2]) / Ks[0, 0], (yy - Ks[1, 2]) / Ks[1, 1], np.ones(len(xx))], -1)
            X = (Z[:, None] * d - t) @ Rm                                            # R^T (P - t)
            rad = np.linalg.norm(X, axis=1)
            tol = ((1 / 512 + 3 * U32 * W) * Z / min(Ks[0, 0], Ks[1, 1]) + 11 * U32 * Z +
                   (0.5 * s["depth_scale"] + 2 * U32 * Z) * np.linalg.norm(d, axis=1) + 2 * U32 * (R0 + np.linalg.norm(t)))
            print("depth_scale", s["depth_scale"], "radius - R max", float((rad - R0).max()), "r_in - radius max", float((r_in - rad).max()),
                  "tolerance min", float(tol.min()))
            assert np.all(rad <= R0 + tol) and np.all(rad >= r_in - tol)


@gpu
def test_meshes_to_a_training_step(golden_dir):
    """Two instances at 480 x 640 -> training_samples -> assemble_training_batch -> the key-point pairs of Net.compute_keypoint_data
    equal oracle.train.keypoint_data's at the tolerance of tests/test_train_gpu.py (<= 0.1 % of the entries differ, each by one pixel
    or by validity) and there are valid pairs (a unit or pose-convention error leaves none); then a train-mode forward, the loss and
    backward() give finite values."""
    from netcfg import small_cfg
    from oracle import train as ot

    from picopose_amd.picopose import Net
    from picopose_amd.utils.loss_utils import Loss

    view_poses = np.load(os.path.join(golden_dir, "template_view_poses_level1.npy"))
    meshes = [ro.cube(half=50.0), ro.icosphere(3, 60.0)]
    obj, img = np.array([0, 1]), np.array([0, 0])
    poses = np.stack([_pose((0.5, 0.3, 0.2), (-70.0, 15.0, 600.0)), _pose((0.2, -0.4, 1.0), (95.0, -20.0, 700.0))])
    rng = np.random.default_rng(12)
    scene = ss.render_scenes(meshes, obj, img, poses, TEMPLATE_K, (480, 640), backgrounds=("lattice", 5, 5), shading=[None, "tless"])
    samples, index = ss.training_samples(scene, poses, obj, img, meshes, view_poses, TEMPLATE_K, rng, return_index=True,
                                         shading=None)
    assert index["instance"].tolist() == [0, 1]
    for s, u in zip(samples, index["instance"]):
        tb.check_sample(s)
        assert s["tem_depth"].dtype == np.uint16 and s["tem_depth"].max() > 1000 and s["rgb"].shape == (480, 640, 3)
    ep = tb.assemble_training_batch(samples, augment_real=False, generator=np.random.default_rng(0))
    torch.manual_seed(0)
    net = Net(small_cfg()).cuda().train()
    got = net.compute_keypoint_data(ep)
    ref = ot.keypoint_data({k: v.detach().cpu().clone() for k, v in ep.items()})
    for k in ("src_pts", "tar_pts"):
        g, r = got[k].cpu(), ref[k]
        assert g.shape == r.shape
        differ = (g != r).any(dim=-1)
        print(k, "entries differing from the oracle:", int(differ.sum()), "of", differ.numel(), "valid:", int((r[..., 0] != -1).sum()))
        assert differ.float().mean() <= 1e-3, (k, int(differ.sum()))
        d = (g[differ] - r[differ]).abs() * 3.5
        assert all(bool((row <= 1.01).all()) or bool((a == -1).all()) or bool((b == -1).all()) for row, a, b in zip(d, g[differ], r[differ]))
    for b in range(2):
        assert int((ref["src_pts"][b, :, 0] != -1).sum()) > 0 and int((got["src_pts"][b, :, 0] != -1).sum()) > 0, b
    res = net(ep)
    tot = Loss()(res)
    assert torch.isfinite(tot["loss"]), {k: float(v) for k, v in res.items() if k.startswith("loss")}
    for k, v in res.items():
        if k.startswith("loss"):
            assert torch.isfinite(v).all(), k
    tot["loss"].backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
