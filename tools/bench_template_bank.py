"""Template-bank onboarding (picopose_amd/provider/template_bank.py), measured:

  * render_templates for 162 views at 480 x 640 on a cube (12 triangles), a 20 k-triangle and a >= 500 k-triangle icosphere:
    host time of the call (it ends with its one device->host copy), HIP events around render_views alone, workspace bytes;
  * the batched crop (templates_from_frames on device-resident frames + the extents copy) against what the per-view helper offers
    for the same job: a loop of utils.preprocess.crop_template over the same 162 frames held as numpy arrays — same process,
    median of --reps after --warmup, synchronised at the ends only;
  * --onboard VIT: onboard_objects for one object split into render / crop / bank features (extended bank with --extended);
  * --profile: one render_templates per mesh and nothing else, for `rocprofv3 --kernel-trace --stats -- python tools/bench_template_bank.py --profile`;
  * --textured WtxHt: the 20 k-triangle icosphere with per-vertex UVs and a generated Wt x Ht texture instead of the three meshes:
    render_templates and render_views for the vertex-colour and the textured path alternately, and the mip pyramid build alone (HIP
    events on the stream); with --profile one textured render_templates and nothing else;
  * --shaded: the 20 k-triangle icosphere's 162 views through render_views unlit, lit flat, lit smooth (precomputed normals), textured
    and textured lit, alternately, twice (HIP events, uploads included: they are the same for every path), and pp_vertex_normals
    alone; with --profile one render of each path and nothing else, for the per-kernel times;
  * --multisample: the 20 k-triangle icosphere's bank (render_templates, 162 views) plain, textured and shading="tless", each with
    samples=1 and samples=4 alternately, twice; with --profile one render_templates of each and nothing else.

Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_oracle as ro  # noqa: E402  (mesh generators only)

from picopose_amd.provider import template_bank as tb  # noqa: E402
from picopose_amd.utils.preprocess import crop_template  # noqa: E402


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
    return statistics.median(out)


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
    return statistics.median(out)


def textured(a, views):
    Wt, Ht = (int(x) for x in a.textured.lower().split("x"))
    m = ro.icosphere(5, 50.0)
    d = m["vertices"].astype(np.float64) / 50.0
    uv = np.stack([np.arctan2(d[:, 1], d[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(d[:, 2], -1, 1)) / np.pi], axis=1).astype(np.float32)
    tex = np.random.default_rng(0).integers(0, 256, (Ht, Wt, 3)).astype(np.uint8)
    tm = {"vertices": m["vertices"], "faces": m["faces"], "uv": uv, "texture": tex}
    if a.profile:
        tb.render_templates(tm, views)
        torch.cuda.synchronize()
        return
    poses = tb.template_object_poses(views, m["vertices"])
    tex_d = torch.from_numpy(tex).cuda()
    for rep in range(2):                                        # the two paths alternately, twice: the spread between the passes is printed
        for name, mesh in (("vertex_colour", m), ("textured", tm)):
            print(json.dumps({"what": "render_templates", "path": name, "pass": rep, "mesh": "icosphere_20480", "views": 162,
                              "texture": a.textured if mesh is tm else None,
                              "host_ms": round(timed(lambda: tb.render_templates(mesh, views), a.reps, a.warmup), 3),
                              "render_views_event_ms": round(events(lambda: tb.render_views(mesh, poses, check_near=False), a.reps, a.warmup), 3)}),
                  flush=True)
    print(json.dumps({"what": "texture_mips alone", "texture": a.textured, "bytes": int(tb.texture_mips(tex_d).numel()),
                      "event_ms": round(events(lambda: tb.texture_mips(tex_d), a.reps, a.warmup), 4)}), flush=True)
    r = tb.render_views(tm, poses, return_face_id=True)
    print(json.dumps({"what": "covered samples", "views": 162, "covered": int((r["face_id"] >= 0).sum().item()),
                      "samples": int(r["face_id"].numel())}), flush=True)


def shaded(a, views):
    m = ro.icosphere(5, 50.0)
    d = m["vertices"].astype(np.float64) / 50.0
    uv = np.stack([np.arctan2(d[:, 1], d[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(d[:, 2], -1, 1)) / np.pi], axis=1).astype(np.float32)
    tm = {"vertices": m["vertices"], "faces": m["faces"], "uv": uv, "texture": np.random.default_rng(0).integers(0, 256, (2048, 2048, 3)).astype(np.uint8)}
    poses = tb.template_object_poses(views, m["vertices"])
    lights = tb.template_lights(tb.mesh_diameter(m["vertices"]) * 1e-3)
    normals = tb.vertex_normals(m).cpu().numpy()                # uploaded per call like the colours: the S8 launch is timed on its own
    paths = {"unlit": (m, None), "lit_flat": (m, dict(lights, normals="flat")), "lit_smooth": (dict(m, normals=normals), dict(lights, normals="smooth")),
             "textured_unlit": (tm, None), "textured_lit_flat": (tm, dict(lights, normals="flat"))}
    if a.profile:
        for mesh, sh in paths.values():
            tb.render_views(mesh, poses, check_near=False, shading=sh)
        tb.vertex_normals(m)
        torch.cuda.synchronize()
        return
    for rep in range(2):
        for name, (mesh, sh) in paths.items():
            print(json.dumps({"what": "render_views", "path": name, "pass": rep, "mesh": "icosphere_20480", "views": 162,
                              "event_ms": round(events(lambda: tb.render_views(mesh, poses, check_near=False, shading=sh), a.reps, a.warmup), 3)}),
                  flush=True)
    print(json.dumps({"what": "vertex_normals alone (CSR built on the host, 4 uploads, one launch)", "vertices": len(m["vertices"]),
                      "event_ms": round(events(lambda: tb.vertex_normals(m), a.reps, a.warmup), 4)}), flush=True)


def multisample(a, views):
    m = ro.icosphere(5, 50.0)
    d = m["vertices"].astype(np.float64) / 50.0
    uv = np.stack([np.arctan2(d[:, 1], d[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(d[:, 2], -1, 1)) / np.pi], axis=1).astype(np.float32)
    tm = {"vertices": m["vertices"], "faces": m["faces"], "uv": uv, "texture": np.random.default_rng(0).integers(0, 256, (2048, 2048, 3)).astype(np.uint8)}
    paths = {"plain": (m, None), "textured": (tm, None), "tless": ({"vertices": m["vertices"], "faces": m["faces"]}, "tless")}
    if a.profile:
        for mesh, sh in paths.values():
            for samples in (1, 4):
                tb.render_templates(mesh, views, shading=sh, samples=samples)
        torch.cuda.synchronize()
        return
    for rep in range(2):
        for name, (mesh, sh) in paths.items():
            ms = {s: timed(lambda: tb.render_templates(mesh, views, shading=sh, samples=s), a.reps, a.warmup) for s in (1, 4)}
            print(json.dumps({"what": "render_templates", "path": name, "pass": rep, "mesh": "icosphere_20480", "views": 162,
                              "samples1_host_ms": round(ms[1], 3), "samples4_host_ms": round(ms[4], 3), "ratio": round(ms[4] / ms[1], 2)}),
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big", type=int, default=8, help="subdivisions of the large icosphere (8: 1 310 720 triangles)")
    ap.add_argument("--onboard", default=None, help="dinov2_vits14 | dinov2_vitb14 | dinov2_vitl14")
    ap.add_argument("--extended", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--textured", default=None, metavar="WtxHt", help="texture size, e.g. 2048x2048")
    ap.add_argument("--shaded", action="store_true")
    ap.add_argument("--multisample", action="store_true")
    a = ap.parse_args()
    views = np.load(os.path.join(ROOT, "tests", "golden", "template_view_poses_level1.npy"))
    if a.textured:
        return textured(a, views)
    if a.shaded:
        return shaded(a, views)
    if a.multisample:
        return multisample(a, views)
    meshes = {"cube_12": ro.cube(40.0), "icosphere_20480": ro.icosphere(5, 50.0)}
    big = ro.icosphere(a.big, 50.0)
    meshes[f"icosphere_{len(big['faces'])}"] = big
    if a.profile:
        for m in meshes.values():
            tb.render_templates(m, views)
        torch.cuda.synchronize()
        return
    for name, m in meshes.items():
        poses = tb.template_object_poses(views, m["vertices"])
        per_view = (480 * 640 + len(m["faces"])) * 8
        chunk = max(1, min(162, (tb.DEFAULT_WORKSPACE_BYTES - 256) // per_view))
        print(json.dumps({"what": "render_templates", "mesh": name, "views": 162,
                          "host_ms": round(timed(lambda: tb.render_templates(m, views), a.reps, a.warmup), 3),
                          "render_views_event_ms": round(events(lambda: tb.render_views(m, poses, check_near=False), a.reps, a.warmup), 3),
                          "workspace_bytes": 256 + chunk * per_view, "views_per_chunk": chunk}), flush=True)
    m = meshes["icosphere_20480"]
    poses = tb.template_object_poses(views, m["vertices"])
    r = tb.render_views(m, poses)
    rgba, depth = r["rgba"].cpu().numpy(), r["depth_mm"].cpu().numpy()
    loop = timed(lambda: [crop_template(rgba[v], depth[v], tb.TEMPLATE_K, poses[v]) for v in range(162)], a.reps, a.warmup)
    batched_np = timed(lambda: tb.templates_from_frames(rgba, depth, tb.TEMPLATE_K, poses), a.reps, a.warmup)
    batched_dev = timed(lambda: tb.templates_from_frames(r["rgba"], r["depth_mm"], tb.TEMPLATE_K, poses), a.reps, a.warmup)
    print(json.dumps({"what": "crop of 162 frames", "crop_template_loop_ms": round(loop, 3),
                      "templates_from_frames_numpy_ms": round(batched_np, 3), "templates_from_frames_device_ms": round(batched_dev, 3),
                      "ratio_numpy_frames": round(loop / batched_np, 2), "ratio_device_frames": round(loop / batched_dev, 2)}), flush=True)
    if a.onboard:
        from picopose_amd.picopose import Net

        ns = types.SimpleNamespace
        C, idx = {"dinov2_vits14": (384, [[0, 2], [3, 5], [6, 8], [9, 11]]), "dinov2_vitb14": (768, [[0, 2], [3, 5], [6, 8], [9, 11]]),
                  "dinov2_vitl14": (1024, [[0, 5], [6, 11], [12, 17], [18, 23]])}[a.onboard]
        cfg = ns(hypothesis=5, stage1=ns(vit_type=a.onboard, pretrained=False, interaction_indexes=idx), stage2=ns(in_channel=256, hidden_dim=256),
                 stage3=ns(nclass=1, in_channels=C, use_bn=True, out_channels=[256, 512, 1024, 1024], num_levels=3, radius=4))
        net = Net(cfg).cuda().eval()
        whole = timed(lambda: tb.onboard_objects(net, [m], views, extended=a.extended), a.reps, a.warmup)
        render = timed(lambda: tb.render_views(m, poses), a.reps, a.warmup)
        bank = timed(lambda: tb.render_templates(m, views), a.reps, a.warmup)
        print(json.dumps({"what": "onboard_objects, one object", "vit": a.onboard, "extended": a.extended, "total_ms": round(whole, 3),
                          "render_ms": round(render, 3), "crop_ms": round(bank - render, 3), "features_ms": round(whole - bank, 3)}), flush=True)


if __name__ == "__main__":
    main()
