"""Synthetic training scenes (picopose_amd/provider/synth_scenes.py), measured: --images x --per-image layers of the 20 480-triangle
icosphere and the cube at 480 x 640, poses from sample_scene_poses (seeded).

  * layer renders: HIP events around the render_views calls that render_scenes makes (one per mesh) — they exist without the
    composite and are the yardstick;
  * composite, the entry alone: HIP events around --inner back-to-back pp_scene_composite calls (its two launches) on device-resident
    layers, with the tables uploaded and the workspace and outputs allocated beforehand; the bytes the algorithm moves — 4 per layer
    sample (depth) + 4 per won pixel (the winner's colour) + 9 per pixel written + 1 per layer sample (the masks) — over the time per
    call, against the 8.0 TB/s HBM peak and the 6.29 TB/s a float4 copy reaches;
  * composite, the whole call: HIP events around composite_layers (layers already sorted by image, so no gather): the same plus the
    tables' uploads, the allocations and the blocking read of the counts — a call time, not a kernel's rate;
  * render_scenes whole (host clock, ends in its device -> host read);
  * training_samples (host clock; template renders, the draws, the device -> host copies of frames, depth and masks) and the copies
    alone;
  * assemble_training_batch of the first --batch samples that follows (host clock to a synchronise).

Median of --reps after --warmup.  --profile: one render_scenes and nothing else, for `rocprofv3 --kernel-trace --stats --`.
Prints one JSON line per measurement."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_oracle as ro  # noqa: E402  (mesh generators only)

from picopose_amd import _lib  # noqa: E402
from picopose_amd.provider import synth_scenes as ss  # noqa: E402
from picopose_amd.provider import template_bank as tb  # noqa: E402
from picopose_amd.provider import training_batch as trb  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out)


def events(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def stats(t):
    return {"ms": round(t[0], 3), "min_ms": round(t[1], 3), "max_ms": round(t[2], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--per-image", type=int, default=4)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back pp_scene_composite calls inside one event pair")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    H, W, K = 480, 640, tb.TEMPLATE_K
    meshes = [ro.icosphere(5, 50.0), ro.cube(40.0)]
    views = np.load(os.path.join(ROOT, "tests", "golden", "template_view_poses_level1.npy"))
    rng = np.random.default_rng(0)
    diam = [100.0, 80.0 * 3 ** 0.5]                                 # the largest vertex distance of the sphere and of the cube, mm
    obj, img, poses = ss.sample_scene_poses(diam, a.images, a.per_image, K, (H, W), rng, size_px=(96.0, 256.0), margin_px=96.0)
    bgs = ("lattice", np.arange(a.images), 5)
    scene_kw = dict(backgrounds=bgs, shading=["tless", None])
    if a.profile:
        ss.render_scenes(meshes, obj, img, poses, K, (H, W), **scene_kw)
        torch.cuda.synchronize()
        return
    shape = {"images": a.images, "layers": len(obj), "H": H, "W": W}

    def renders():
        return [tb.render_views(meshes[m], poses[obj == m], K=K, resolution=(H, W), return_depth_m=True, check_near=False,
                                shading=scene_kw["shading"][m]) for m in (0, 1)]

    print(json.dumps({"what": "layer renders (render_views, one call per mesh)", **shape, **stats(events(renders, a.reps, a.warmup))}), flush=True)
    r = renders()
    rgba = torch.empty((len(obj), H, W, 4), dtype=torch.uint8, device="cuda")
    depth = torch.empty((len(obj), H, W), dtype=torch.float32, device="cuda")
    for m in (0, 1):
        at = torch.from_numpy(np.nonzero(obj == m)[0]).cuda()
        rgba.index_copy_(0, at, r[m]["rgba"])
        depth.index_copy_(0, at, r[m]["depth_m"])
    del r
    order, off = ss._layer_order(img, len(obj), a.images)
    assert np.array_equal(order, np.arange(len(obj)))              # sample_scene_poses gives the instances image by image
    desc, _ = ss.background_table(bgs, a.images, H, W)
    scales = ss._scales(0.1, a.images)
    off_d, desc_d, sc_d = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (off, desc, scales))
    lib, need = _lib.lib(), ctypes.c_size_t()
    _lib.check(lib.pp_scene_composite_workspace_bytes(len(obj), H, W, ctypes.byref(need)), "pp_scene_composite_workspace_bytes")
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda")
    out = ss._outputs(a.images, len(obj), H, W, True, torch.device("cuda"))
    for masks in (True, False):
        comp = ss.composite_layers(rgba, depth, img, a.images, backgrounds=bgs, masks=masks)
        won = int(comp["px_count_visib"].sum().item())
        moved = len(obj) * H * W * (4 + (1 if masks else 0)) + 4 * won + 9 * a.images * H * W

        def entry():
            for _ in range(a.inner):
                _lib.check(lib.pp_scene_composite(rgba.data_ptr(), depth.data_ptr(), off_d.data_ptr(), off.ctypes.data, len(obj), a.images, H, W,
                                                  desc_d.data_ptr(), desc.ctypes.data, None, sc_d.data_ptr(), scales.ctypes.data, ws.data_ptr(),
                                                  ws.numel(), out["rgb"].data_ptr(), out["depth"].data_ptr(), out["instance"].data_ptr(),
                                                  out["counts"].data_ptr(), out["boxes"].data_ptr(),
                                                  out["mask"].data_ptr() if masks else None, _lib.stream_ptr()), "pp_scene_composite")

        t = tuple(v / a.inner for v in events(entry, a.reps, a.warmup))
        print(json.dumps({"what": "composite, the entry alone (pp_scene_composite: two launches; per call, %d calls per event pair)" % a.inner,
                          "masks": masks, **shape, **stats(t), "algorithmic_bytes": moved, "won_pixels": won,
                          "bytes_per_s": round(moved / (t[0] * 1e-3), 1), "share_of_hbm_peak": round(moved / (t[0] * 1e-3) / HBM_PEAK, 4),
                          "share_of_float4_copy_rate": round(moved / (t[0] * 1e-3) / HBM_COPY, 4)}), flush=True)
        t = events(lambda: ss.composite_layers(rgba, depth, img, a.images, backgrounds=bgs, masks=masks), a.reps, a.warmup)
        print(json.dumps({"what": "composite, the whole call (composite_layers: uploads, allocations, pp_scene_composite, the counts' read)",
                          "masks": masks, **shape, **stats(t)}), flush=True)
    whole = timed(lambda: ss.render_scenes(meshes, obj, img, poses, K, (H, W), **scene_kw), a.reps, a.warmup)
    print(json.dumps({"what": "render_scenes whole (host clock)", **shape, **stats(whole)}), flush=True)
    scene = ss.render_scenes(meshes, obj, img, poses, K, (H, W), **scene_kw)
    kept = int(((scene["px_count_all"].cpu().numpy() >= ss.MIN_VISIB_PX) & (scene["visib_fract"] >= ss.MIN_VISIB_FRACT)).sum())
    t = timed(lambda: ss.training_samples(scene, poses, obj, img, meshes, views, K, np.random.default_rng(1), shading=None), a.reps, a.warmup)
    copies = timed(lambda: (scene["rgb"].cpu(), scene["depth"].cpu(), scene["mask_visib"].cpu()), a.reps, a.warmup)
    print(json.dumps({"what": "training_samples (host clock; template renders and device -> host copies included)", **shape, "kept": kept,
                      **stats(t), "device_to_host_copies_alone_ms": round(copies[0], 3),
                      "copied_bytes": int(scene["rgb"].numel() + 2 * scene["depth"].numel() + scene["mask_visib"].numel())}), flush=True)
    samples = ss.training_samples(scene, poses, obj, img, meshes, views, K, np.random.default_rng(1), shading=None)[:a.batch]
    t = timed(lambda: trb.assemble_training_batch(samples, generator=np.random.default_rng(2)), a.reps, a.warmup)
    print(json.dumps({"what": "assemble_training_batch of the samples (host clock)", "batch": len(samples), **stats(t)}), flush=True)


if __name__ == "__main__":
    main()
