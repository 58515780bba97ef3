"""Synthetic training pairs from meshes alone: rendered multi-object scenes with mutual occlusion over a background, cut into the
decoded pairs that provider.training_batch.assemble_training_batch takes.

    obj, img, poses = sample_scene_poses(diameters_mm, n_images, per_image, K, (H, W), rng)
    scene = render_scenes(meshes, obj, img, poses, K, (H, W), backgrounds=("lattice", seeds, 5), shading="tless")
    samples = training_samples(scene, poses, obj, img, meshes, view_poses, K, rng)
    end_points = assemble_training_batch(samples, generator=rng)          # -> Net.forward in train mode

Every object instance is rendered into a full-frame LAYER by template_bank.render_views (unlit, textured or shaded); the layers of an
image are composited by pp_scene_composite (csrc/pp_synth.hip, "THE SCENE COMPOSITE" of include/picopose_hip.h): per pixel the
nearest layer wins, the frame takes its colour or the background's, and per instance come the covered and visible pixel counts, the
box and the visible mask.  tests/synth_oracle.py restates the composite in numpy, bit for bit.

Stated deviations from the reference's training data (MegaPose's BlenderProc renders): these are domain-randomised rasteriser
frames.  Silhouettes are not anti-aliased and there are no shadows or inter-reflections; appearance variation comes from `shading=`,
the backgrounds and training_batch.ColorAugmentor.  Whether a network fine-tuned on them improves on real images is not measured
here and is not claimed.  The samples go to the host because assemble_training_batch takes host arrays; a device-resident hand-off
is out of scope."""
import numpy as np
import torch

from .. import _lib
from .template_bank import (DEFAULT_WORKSPACE_BYTES, TEMPLATE_K, _mesh_arrays, _raise_on_near, _unit_scale, render_views,
                            template_object_poses)
from .training_batch import nearest_template_views

BG_WORDS, TILE = _lib.PP_SYNTH_BG_WORDS, _lib.PP_SYNTH_TILE
MIN_VISIB_PX, MIN_VISIB_FRACT = 1024, 0.3    # config/base.yaml: min_px_count_visib, min_visib_fract
TEMPLATE_UNITS_PER_METRE = 10000.0       # the template depth files' 0.1 mm unit (training_dataset.py:294)


def _is_triple(b):
    return (isinstance(b, (tuple, list, np.ndarray)) and len(b) == 3 and
            all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in b))


def _one_background(b, H, W):
    """One image's background -> (descriptor words, (H, W, 3) uint8 array or None)."""
    if b is None:
        b = (128, 128, 128)
    if _is_triple(b):
        if not all(0 <= int(v) <= 255 for v in b):
            raise ValueError(f"a background colour must hold three values in 0..255, got {tuple(b)!r}")
        return [0, int(b[0]) | int(b[1]) << 8 | int(b[2]) << 16, 0, 0], None
    if isinstance(b, tuple) and len(b) == 3 and b[0] == "lattice":
        seed, s = int(b[1]), b[2]
        if not (isinstance(s, (int, np.integer)) and 2 <= int(s) <= 7):
            raise ValueError(f"a lattice background's cell_log2 must be an int in 2..7, got {s!r}")
        return [2, int(np.uint32(seed & 0xFFFFFFFF).view(np.int32)), int(s), 0], None
    a = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    if a.shape != (H, W, 3) or a.dtype != np.uint8:
        raise ValueError(f"a background image must be ({H}, {W}, 3) uint8, got {a.dtype} {a.shape}")
    return [1, 0, 0, 0], a


def background_table(backgrounds, n_images, H, W):
    """`backgrounds` -> (descriptors (n_images, 4) int32, images (n_images, H, W, 3) uint8 or None).  None: mid-grey (128, 128, 128);
    an RGB triple of ints; an (n_images, H, W, 3) uint8 array or tensor; ("lattice", seeds, cell_log2) with seeds an int or (n_images,)
    and cell_log2 an int in 2..7 or (n_images,); or a list of n_images entries, each None, a triple, an (H, W, 3) array or
    ("lattice", seed, cell_log2).  A device tensor of images is used where it lies."""
    desc = np.zeros((n_images, BG_WORDS), np.int32)
    if isinstance(backgrounds, tuple) and len(backgrounds) == 3 and isinstance(backgrounds[0], str):
        if backgrounds[0] != "lattice":
            raise ValueError(f"unknown background {backgrounds[0]!r}")
        seeds = np.broadcast_to(np.asarray(backgrounds[1], dtype=np.int64), (n_images,))
        cells = np.asarray(backgrounds[2])
        if not np.issubdtype(cells.dtype, np.integer):
            raise ValueError(f"a lattice background's cell_log2 must be an int in 2..7, got {backgrounds[2]!r}")
        cells = np.broadcast_to(cells, (n_images,))
        for i in range(n_images):
            desc[i] = _one_background(("lattice", int(seeds[i]), int(cells[i])), H, W)[0]
        return desc, None
    if backgrounds is None or _is_triple(backgrounds):
        desc[:] = _one_background(backgrounds, H, W)[0]
        return desc, None
    if isinstance(backgrounds, list):
        if len(backgrounds) != n_images:
            raise ValueError(f"{len(backgrounds)} backgrounds for {n_images} images")
        images = None
        for i, b in enumerate(backgrounds):
            d, a = _one_background(b, H, W)
            desc[i] = d
            if a is not None:
                if images is None:
                    images = np.zeros((n_images, H, W, 3), np.uint8)
                images[i] = a
        return desc, images
    shape = tuple(backgrounds.shape) if hasattr(backgrounds, "shape") else None
    is_u8 = backgrounds.dtype == torch.uint8 if isinstance(backgrounds, torch.Tensor) else getattr(backgrounds, "dtype", None) == np.uint8
    if shape != (n_images, H, W, 3) or not is_u8:
        raise ValueError(f"background images must be ({n_images}, {H}, {W}, 3) uint8, got {shape}")
    desc[:, 0] = 1
    return desc, backgrounds


def _scales(depth_scale, n_images):
    s = np.array(np.broadcast_to(np.asarray(depth_scale, dtype=np.float32), (n_images,)))          # (a writable copy)
    if not np.all(np.isfinite(s) & (s > 0)):
        raise ValueError("depth_scale must be positive and finite")
    return s


def _composite_call(rgba, depth_m, off, desc, bg_images, scales, H, W, out, l0, i0, masks):
    """One pp_scene_composite call: layers [l0, l0 + L) (sorted by image) onto images [i0, i0 + n) of the output tensors."""
    L_, n = int(off[-1]), len(off) - 1
    dev = out["rgb"].device
    ws = torch.empty(max(_lib.workspace_bytes("pp_scene_composite_workspace_bytes", L_, H, W), 256), dtype=torch.uint8, device=dev)
    off = np.ascontiguousarray(off, dtype=np.int32)
    desc = np.ascontiguousarray(desc, dtype=np.int32)
    scales = np.ascontiguousarray(scales, dtype=np.float32)
    off_d, desc_d, sc_d = (torch.from_numpy(a).to(dev) for a in (off, desc, scales))
    _lib.call("pp_scene_composite", rgba if L_ else None, depth_m if L_ else None, off_d, off, L_, n, H, W, desc_d, desc, bg_images, sc_d,
              scales, ws, ws.numel(), out["rgb"][i0:], out["depth"][i0:], out["instance"][i0:], out["counts"][l0:] if L_ else None,
              out["boxes"][l0:] if L_ else None, out["mask"][l0:] if masks and L_ else None)


def _outputs(n_images, L_, H, W, masks, dev):
    return {"rgb": torch.empty((n_images, H, W, 3), dtype=torch.uint8, device=dev),
            "depth": torch.empty((n_images, H, W), dtype=torch.uint16, device=dev),
            "instance": torch.empty((n_images, H, W), dtype=torch.int32, device=dev),
            "counts": torch.empty((L_, 2), dtype=torch.int32, device=dev), "boxes": torch.empty((L_, 4), dtype=torch.int32, device=dev),
            "mask": torch.empty((L_, H, W), dtype=torch.uint8, device=dev) if masks else None}


def _finish(out, order, masks, extra=None):
    """Sorted layer order -> the caller's: per-layer rows scattered back, instance indices mapped through `order`.  The counts go to
    the host for visib_fract in the call's ONE device -> host read; `extra` (an int32 device tensor) rides in the same copy and comes
    back as res["_extra"] (numpy)."""
    dev, U = out["rgb"].device, len(order)
    counts, boxes, mask, inst = out["counts"], out["boxes"], out["mask"], out["instance"]
    if U and not np.array_equal(order, np.arange(U)):
        inv = torch.from_numpy(np.argsort(order, kind="stable")).to(dev)
        counts, boxes = counts[inv], boxes[inv]
        mask = None if mask is None else mask[inv]
        label = torch.from_numpy(np.concatenate([[-1], order]).astype(np.int32)).to(dev)
        inst = label[(inst + 1).long()]
    tail = torch.zeros(0, dtype=torch.int32, device=dev) if extra is None else extra.reshape(-1)
    host = torch.cat([counts.reshape(-1), tail]).cpu().numpy()     # the one device -> host read
    c = host[:2 * U].reshape(U, 2).astype(np.float64)
    res = {"rgb": out["rgb"], "depth": out["depth"], "instance_map": inst, "px_count_all": counts[:, 0], "px_count_visib": counts[:, 1],
           "bbox_visib": boxes, "visib_fract": np.divide(c[:, 1], c[:, 0], out=np.zeros(U, dtype=np.float64), where=c[:, 0] > 0)}
    if masks:
        res["mask_visib"] = mask
    if extra is not None:
        res["_extra"] = host[2 * U:]
    return res


def _layer_order(layer_image, U, n_images):
    img = np.asarray(layer_image, dtype=np.int64).reshape(-1)
    if len(img) != U:
        raise ValueError(f"{len(img)} image indices for {U} layers")
    if U and (img.min() < 0 or img.max() >= n_images):
        raise ValueError(f"an image index lies outside [0, {n_images})")
    order = np.argsort(img, kind="stable")
    off = np.zeros(n_images + 1, dtype=np.int32)
    np.cumsum(np.bincount(img, minlength=n_images), out=off[1:])
    return order, off


def composite_layers(rgba, depth_m, layer_image, n_images, backgrounds=None, depth_scale=0.1, masks=True, device="cuda"):
    """Composite L rendered layers onto n_images frames in one pp_scene_composite call.  rgba (L, H, W, 4) uint8 and depth_m (L, H, W)
    float32 metres (render_views' "rgba" and "depth_m"; 0, a negative value or a NaN does not cover; alpha is not read), tensors or
    arrays; layer_image (L,) the image of each layer, in any order: the layers are sorted stably by image for the call and every
    per-layer result is scattered back.  backgrounds: see background_table.  depth_scale: a number or (n_images,), millimetres per
    depth unit (the camera.json value: 0.1 gives 0.1 mm units).  ->
      {"rgb" (n_images, H, W, 3) uint8, "depth" (n_images, H, W) uint16 = min(65535, rint(1000 Z / depth_scale)) (0: background),
       "instance_map" (n_images, H, W) int32: the index IN THE CALLER'S ORDER of the nearest layer (on equal depth the one that comes
       first among the image's layers), -1 = background, "px_count_all", "px_count_visib" (L,) int32, "bbox_visib" (L, 4) int32
       inclusive corners ({0, 0, -1, -1}: nothing visible), "mask_visib" (L, H, W) uint8 0 / 255 with masks=True — device tensors;
       "visib_fract" (L,) float64 numpy = px_count_visib / px_count_all, 0 where nothing is covered}."""
    rgba_d = torch.as_tensor(rgba).to(device).contiguous()
    depth_d = torch.as_tensor(depth_m).to(device).contiguous()
    if rgba_d.dim() != 4 or rgba_d.shape[-1] != 4 or rgba_d.dtype != torch.uint8:
        raise ValueError(f"rgba must be (L, H, W, 4) uint8, got {rgba_d.dtype} {tuple(rgba_d.shape)}")
    if depth_d.dtype != torch.float32 or tuple(depth_d.shape) != tuple(rgba_d.shape[:3]):
        raise ValueError(f"depth_m must be float32 {tuple(rgba_d.shape[:3])}, got {depth_d.dtype} {tuple(depth_d.shape)}")
    U, H, W = (int(v) for v in depth_d.shape)
    if not (isinstance(n_images, (int, np.integer)) and n_images > 0) or H <= 0 or W <= 0:
        raise ValueError("n_images, H and W must be positive")
    if max(U, n_images) * H * W >= 2 ** 31:
        raise ValueError("layers or frames too large for 32-bit pixel offsets: split the images over calls")
    order, off = _layer_order(layer_image, U, n_images)
    desc, bg = background_table(backgrounds, n_images, H, W)
    bg_d = None if bg is None else torch.as_tensor(bg).to(device).contiguous()
    scales = _scales(depth_scale, n_images)
    if U and not np.array_equal(order, np.arange(U)):
        idx = torch.from_numpy(order).to(rgba_d.device)
        rgba_d, depth_d = rgba_d[idx], depth_d[idx]
    out = _outputs(n_images, U, H, W, masks, rgba_d.device)
    _composite_call(rgba_d, depth_d, off, desc, bg_d, scales, H, W, out, 0, 0, masks)
    return _finish(out, order, masks)


def image_groups(off, layer_bytes, workspace_bytes):
    """Ranges [i0, i1) of WHOLE images whose layers fit `workspace_bytes` at `layer_bytes` each.  ValueError when one image alone
    does not fit."""
    groups, n, i0 = [], len(off) - 1, 0
    for i in range(n):
        mine = int(off[i + 1] - off[i]) * layer_bytes
        if mine > workspace_bytes:
            raise ValueError(f"the {int(off[i + 1] - off[i])} layers of image {i} need {mine} bytes: more than workspace_bytes = "
                             f"{workspace_bytes}")
        if int(off[i + 1] - off[i0]) * layer_bytes > workspace_bytes:
            groups.append((i0, i))
            i0 = i
    groups.append((i0, n))
    return groups


def render_scenes(meshes, obj_index, image_index, poses_mm, K, resolution, n_images=None, backgrounds=None, shading=None, units="mm",
                  depth_scale=0.1, near=1e-3, masks=True, workspace_bytes=DEFAULT_WORKSPACE_BYTES,
                  render_workspace_bytes=DEFAULT_WORKSPACE_BYTES, device="cuda"):
    """Render U object instances into n_images scenes.  meshes: a list of render_views mesh dicts; obj_index (U,) indexes it;
    image_index (U,) the image of each instance (n_images defaults to its maximum + 1; an image may hold no instance); poses_mm
    (U, 4, 4) object -> camera with the translation in the meshes' `units`; K (3, 3) shared by the images; resolution (H, W).
    shading: one render_views value for every mesh, or a list with one per mesh.  backgrounds, depth_scale, masks: composite_layers'.

    The instances are ordered stably by image and cut into groups of whole images whose layers fit `workspace_bytes` — the layers
    themselves count, 8 bytes per layer sample (plus the mask byte and the composite's records).  Per group there is one
    render_views(..., return_depth_m=True, check_near=False) call per distinct mesh (one per mesh when everything fits one group) and
    one pp_scene_composite call; the results do not depend on the grouping.  `workspace_bytes` bounds the layer buffers of a group
    and nothing else: each render_views call works inside its own `render_workspace_bytes` (that function's workspace_bytes) and
    returns its frames in buffers of its own (10 bytes per sample of that mesh's instances in the group) before they are copied into
    the group's, so the peak device memory of a group is up to twice `workspace_bytes` plus `render_workspace_bytes`, on top of the
    outputs.  ValueError when a triangle reaches the near plane (`near` metres), exactly as render_templates raises it, after the
    one device -> host read at the end (the pixel counts and the near-plane count in one copy).
    -> composite_layers' result with "instance_map" in the caller's instance order, plus "n_groups".  px_count_all counts IN-FRAME
    pixels only: the visible fraction of an object cut by the frame border is therefore higher than BOP's padded-canvas value from
    scene_gt.scene_gt_info(pad="bop")."""
    obj = np.asarray(obj_index, dtype=np.int64).reshape(-1)
    U = len(obj)
    poses = np.asarray(poses_mm, dtype=np.float64)
    if poses.shape != (U, 4, 4):
        raise ValueError(f"poses_mm must be ({U}, 4, 4), got {poses.shape}")
    if U and (obj.min() < 0 or obj.max() >= len(meshes)):
        raise ValueError(f"an obj_index lies outside the {len(meshes)} meshes")
    H, W = int(resolution[0]), int(resolution[1])
    img = np.asarray(image_index, dtype=np.int64).reshape(-1)
    if n_images is None:
        n_images = int(img.max()) + 1 if U else 1
    if n_images <= 0 or H <= 0 or W <= 0 or n_images * H * W >= 2 ** 31:
        raise ValueError("n_images, H and W must be positive with n_images H W < 2^31")
    shadings = list(shading) if isinstance(shading, list) else [shading] * len(meshes)
    if len(shadings) != len(meshes):
        raise ValueError(f"{len(shadings)} shadings for {len(meshes)} meshes")
    order, off = _layer_order(img, U, n_images)
    desc, bg = background_table(backgrounds, n_images, H, W)
    bg_d = None if bg is None else torch.as_tensor(bg).to(device).contiguous()
    scales = _scales(depth_scale, n_images)
    layer_bytes = H * W * (8 + (1 if masks else 0)) + 24 * ((H * W + TILE - 1) // TILE)
    groups = image_groups(off, layer_bytes, int(workspace_bytes))
    out = _outputs(n_images, U, H, W, masks, torch.device(device))
    near_total = torch.zeros(1, dtype=torch.int32, device=device)
    s_obj, s_pose = obj[order], poses[order]
    for i0, i1 in groups:
        l0, l1 = int(off[i0]), int(off[i1])
        n_l = l1 - l0
        if n_l * H * W >= 2 ** 31:
            raise ValueError("a group's layers exceed 32-bit pixel offsets: lower workspace_bytes")
        rgba = torch.empty((n_l, H, W, 4), dtype=torch.uint8, device=device)
        depth_m = torch.empty((n_l, H, W), dtype=torch.float32, device=device)
        for m in np.unique(s_obj[l0:l1]):
            rows = np.nonzero(s_obj[l0:l1] == m)[0]
            r = render_views(meshes[int(m)], s_pose[l0:l1][rows], K=K, resolution=(H, W), units=units, near=near, return_depth_m=True,
                             workspace_bytes=render_workspace_bytes, check_near=False, device=device, shading=shadings[int(m)])
            at = torch.from_numpy(rows).to(device)
            rgba.index_copy_(0, at, r["rgba"])
            depth_m.index_copy_(0, at, r["depth_m"])
            near_total += r["near_count"]
        _composite_call(rgba, depth_m, off[i0:i1 + 1] - off[i0], desc[i0:i1], None if bg_d is None else bg_d[i0:i1], scales[i0:i1], H, W,
                        out, l0, i0, masks)
        if l0:                                                     # the call's layer indices -> indices of the sorted order
            view = out["instance"][i0:i1]
            view += (view >= 0).to(torch.int32) * l0
    res = _finish(out, order, masks, extra=near_total)           # the counts and the near-plane count: one device -> host copy
    _raise_on_near(int(res.pop("_extra")[0]), near)
    res["n_groups"] = len(groups)
    return res


def _random_rotations(generator, n):
    """Uniform rotations: a normalised 4-vector of normals as a unit quaternion (w, x, y, z) -> (n, 3, 3)."""
    q = generator.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def sample_scene_poses(diameters_mm, n_images, per_image, K, resolution, generator, size_px=(96.0, 256.0), margin_px=32.0, near=1.0):
    """Random instances for render_scenes, host numpy.  diameters_mm (n_objects,); per_image: the instances of every image, an int or an
    inclusive (lo, hi) range drawn per image; the object of an instance is uniform over the objects.  Rotations are uniform (a
    normalised 4-vector of normals as a quaternion).  The distance follows from the projected diameter s ~ U(size_px) pixels:
    Z = f d / s with f = (fx + fy) / 2.  The projected centre (u, v) is uniform in the frame shrunk by margin_px,
    [margin, W - 1 - margin] x [margin, H - 1 - margin], and X = (u - cx) Z / fx, Y = (v - cy) Z / fy.  Millimetres.
    ValueError when size_px would put Z - d / 2 at or under the near plane (`near`, mm: render_views' 1e-3 m) for an object, when
    size_px is not 0 < lo <= hi, or when the margin empties the frame.  The same Generator state gives the same draws.
    -> obj_index (U,) int64, image_index (U,) int64 (ascending), poses_mm (U, 4, 4) float64."""
    d = np.asarray(diameters_mm, dtype=np.float64).reshape(-1)
    if len(d) == 0 or not np.all(np.isfinite(d) & (d > 0)):
        raise ValueError("diameters_mm must hold positive finite values")
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    H, W = int(resolution[0]), int(resolution[1])
    lo, hi = (float(v) for v in size_px)
    if not (0 < lo <= hi):
        raise ValueError(f"size_px must be 0 < lo <= hi, got {size_px!r}")
    f = 0.5 * (fx + fy)
    if np.any(f * d / hi - 0.5 * d <= near):
        raise ValueError(f"size_px = {size_px!r} puts an object's front (Z - d / 2) at or under the near plane ({near} mm)")
    m = float(margin_px)
    if m < 0 or W - 1 - 2 * m < 0 or H - 1 - 2 * m < 0:
        raise ValueError(f"margin_px = {margin_px!r} empties the {H} x {W} frame")
    if n_images <= 0:
        raise ValueError("n_images must be positive")
    if isinstance(per_image, (int, np.integer)):
        count = np.full(n_images, int(per_image), dtype=np.int64)
    else:
        c_lo, c_hi = (int(v) for v in per_image)
        if not 0 <= c_lo <= c_hi:
            raise ValueError(f"per_image must be an int or 0 <= lo <= hi, got {per_image!r}")
        count = generator.integers(c_lo, c_hi + 1, n_images)
    if count.min() < 0:
        raise ValueError("per_image must not be negative")
    U = int(count.sum())
    image_index = np.repeat(np.arange(n_images, dtype=np.int64), count)
    obj_index = generator.integers(0, len(d), U).astype(np.int64)
    R = _random_rotations(generator, U)
    s = generator.uniform(lo, hi, U)
    u = generator.uniform(m, W - 1 - m, U)
    v = generator.uniform(m, H - 1 - m, U)
    Z = f * d[obj_index] / s
    poses = np.tile(np.eye(4), (U, 1, 1))
    poses[:, :3, :3] = R
    poses[:, 0, 3], poses[:, 1, 3], poses[:, 2, 3] = (u - cx) * Z / fx, (v - cy) * Z / fy, Z
    return obj_index, image_index, poses


def template_frame_poses(mesh, view_ids, view_poses, units="mm"):
    """The object poses of the template views `view_ids` (template_object_poses: the view's rotation, t = (0, 0, diameter)) ->
    (render poses (n, 4, 4) with t in the mesh's units, tem_pose (n, 4, 4) with t in 0.1 mm — the stored template convention:
    t * 0.1 / 1000 is metres, as training_batch._prepare applies it)."""
    v = _mesh_arrays(mesh)[0]
    ids = np.asarray(view_ids, dtype=np.int64).reshape(-1)
    poses = template_object_poses(np.asarray(view_poses)[ids], v)
    tem = poses.copy()
    tem[:, :3, 3] *= _unit_scale(units, v) * TEMPLATE_UNITS_PER_METRE
    return poses, tem


def depth_quantize_u16(depth_m, units_per_metre):
    """pp_depth_quantize_u16 on a float32 device tensor: Z > 0 ? min(65535, rint(units_per_metre Z)) : 0 -> uint16, same shape."""
    if not depth_m.is_cuda or depth_m.dtype != torch.float32:
        raise ValueError("depth_m must be a float32 device tensor")
    depth_m = depth_m.contiguous()
    out = torch.empty(depth_m.shape, dtype=torch.uint16, device=depth_m.device)
    _lib.call("pp_depth_quantize_u16", depth_m, depth_m.numel(), float(units_per_metre), out)
    return out


def render_template_frames(mesh, view_ids, view_poses, K=TEMPLATE_K, resolution=(480, 640), units="mm", shading=None, device="cuda"):
    """The template frames of one object as the reference's template files hold them: render_views at template_object_poses of the
    views `view_ids` of view_poses (V, 4, 4) -> {"tem_rgba" (n, H, W, 4) uint8 and "tem_depth" (n, H, W) uint16 in 0.1 mm
    (pp_depth_quantize_u16 with 10000) device tensors, "tem_pose" (n, 4, 4) float64 numpy with t in 0.1 mm}."""
    poses, tem = template_frame_poses(mesh, view_ids, view_poses, units)
    r = render_views(mesh, poses, K=K, resolution=resolution, units=units, return_depth_m=True, device=device, shading=shading)
    return {"tem_rgba": r["rgba"], "tem_depth": depth_quantize_u16(r["depth_m"], TEMPLATE_UNITS_PER_METRE), "tem_pose": tem}


def _host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def training_samples(scene, poses_mm, obj_index, image_index, meshes, view_poses, K, generator, min_visib_px=MIN_VISIB_PX,
                     min_visib_fract=MIN_VISIB_FRACT, topk=5, depth_scale=0.1, template_K=TEMPLATE_K, render_frames=None,
                     return_index=False, **template_kw):
    """Cut render_scenes' result into the decoded pairs of assemble_training_batch.  scene: that result (masks=True), tensors or
    arrays; poses_mm (U, 4, 4) with t in millimetres, obj_index, image_index, meshes, depth_scale: what render_scenes was given
    (depth_scale a number or (n_images,)); view_poses (V, 4, 4): the template views; K (3, 3).
    An instance is kept by the rule of training_dataset.py:178 with the reference's config/base.yaml defaults: px_count_valid >=
    min_visib_px and visib_fract >= min_visib_fract — every covered pixel of a rendered scene has a depth, so px_count_valid is
    px_count_all — and, as :199, a non-empty visible mask.  Per kept instance the template view is a Generator draw among
    training_batch.nearest_template_views(R, view_poses, topk); the template frames are rendered once per distinct (mesh, view) by
    render_template_frames(mesh, view_ids, view_poses, K=template_K, **template_kw).  template_K is the template camera (the scene's
    K is a positional argument of this function, so the template's cannot travel in template_kw).  render_frames: a callable
    (mesh, view_ids) -> render_template_frames' dict, used instead of it — for template frames that come from elsewhere (files of a
    dataset, another renderer; the tests pass a CPU renderer).
    -> a list of dicts with exactly the keys training_batch._prepare reads: rgb, mask, depth, depth_scale, K, cam_R_m2c, cam_t_m2c,
    tem_rgba, tem_depth, tem_pose, templates_K (= template_K); with return_index=True also {"instance", "view"}
    arrays, one entry per sample.  The arrays go to the host here (frames of one image are shared between its samples, not copied):
    assemble_training_batch takes host arrays."""
    obj = np.asarray(obj_index, dtype=np.int64).reshape(-1)
    img = np.asarray(image_index, dtype=np.int64).reshape(-1)
    poses = np.asarray(poses_mm, dtype=np.float64)
    U = len(obj)
    if "mask_visib" not in scene:
        raise ValueError("training_samples needs the scene's mask_visib: render_scenes(..., masks=True)")
    n_all, n_vis = _host(scene["px_count_all"]), _host(scene["px_count_visib"])
    fract = np.asarray(scene["visib_fract"], dtype=np.float64)
    if not (len(img) == len(poses) == len(n_all) == U) or poses.shape[1:] != (4, 4):
        raise ValueError("obj_index, image_index, poses_mm and the scene disagree on the number of instances")
    keep = np.nonzero((n_all >= min_visib_px) & (fract >= min_visib_fract) & (n_vis > 0))[0]
    view_poses = np.asarray(view_poses)
    views = np.zeros(len(keep), dtype=np.int64)
    for k, u in enumerate(keep):
        ids = nearest_template_views(poses[u, :3, :3], view_poses, topk)
        views[k] = ids[int(generator.integers(len(ids)))]
    if render_frames is None:
        render_frames = lambda mesh, ids: render_template_frames(mesh, ids, view_poses, K=template_K, **template_kw)      # noqa: E731
    frames = {}                                                   # (mesh, view) -> (rgba, depth, pose), each rendered once
    for m in np.unique(obj[keep]):
        ids = np.unique(views[obj[keep] == m])
        r = render_frames(meshes[int(m)], ids)
        rgba, dep, pose = _host(r["tem_rgba"]), _host(r["tem_depth"]), np.asarray(r["tem_pose"], dtype=np.float64)
        for j, vid in enumerate(ids):
            frames[(int(m), int(vid))] = (rgba[j], dep[j], pose[j])
    mask = scene["mask_visib"]
    if isinstance(mask, torch.Tensor):
        mask = mask[torch.from_numpy(keep).to(mask.device)].cpu().numpy()
    else:
        mask = np.asarray(mask)[keep]
    rgb, depth = _host(scene["rgb"]), _host(scene["depth"])
    scales = np.broadcast_to(np.asarray(depth_scale, dtype=np.float64), (len(rgb),))
    tK = np.asarray(template_K, dtype=np.float64).reshape(3, 3)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    samples = []
    for k, u in enumerate(keep):
        t_rgba, t_depth, t_pose = frames[(int(obj[u]), int(views[k]))]
        i = int(img[u])
        samples.append({"rgb": rgb[i], "mask": mask[k], "depth": depth[i], "depth_scale": float(scales[i]), "K": K,
                        "cam_R_m2c": poses[u, :3, :3].reshape(9).copy(), "cam_t_m2c": poses[u, :3, 3].copy(), "tem_rgba": t_rgba,
                        "tem_depth": t_depth, "tem_pose": t_pose.copy(), "templates_K": tK})
    if return_index:
        return samples, {"instance": keep, "view": views}
    return samples
