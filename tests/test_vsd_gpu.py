"""GPU: pp_vsd_errors (picopose_amd/evaluation.py: vsd_errors, render_depth, match_and_score with depth images) against
tests/vsd_oracle.py: depth renders bit-equal to the windowed raster restatement, window "auto" bit-equal to "full", counts equal and
errors bit-equal to the float32 restatement, counts within the fragile pixels of the float64 definition, the closed-form plate scenes
through the kernel, edge shapes, determinism across streams, pair order and grouping, and the recalls and AR end to end."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_error_oracle as po  # noqa: E402
import render_oracle as ro  # noqa: E402
import vsd_oracle as vo  # noqa: E402

from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import scene as scn  # noqa: E402
from picopose_amd.evaluation import vsd_errors  # noqa: E402,F401  (absent before the feature)

gpu = pytest.mark.gpu
F = np.float32
KEYS = ("vsd", "visib_union", "visib_inter", "n_far")


@functools.lru_cache(maxsize=None)
def _mixed():
    """The mixed scene and the oracle's answer, computed once and shared (never modified)."""
    scene = vo.mixed_scene()
    return scene, vo.reference(scene)


def _models(scene):
    return ev.ObjectModels(scene["objects"])


def _run(models, scene, rows=None, **kw):
    rows = np.arange(len(scene["obj_ids"])) if rows is None else rows
    depth = {"depth": scene["depth_mm"]} if "depth_mm" in scene else {"depth": scene["depth_u16"], "depth_scale": scene["depth_scale"]}
    r = ev.vsd_errors(models, scene["obj_ids"][rows], scene["R_est"][rows], scene["t_est"][rows], scene["R_gt"][rows], scene["t_gt"][rows],
                      scene["K"], image_index=scene["image_index"][rows], **depth, **kw)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _counts(got):
    return np.concatenate([got["visib_union"][:, None], got["visib_inter"][:, None], got["n_far"]], axis=1).astype(np.int64)


def _assert_equals_oracle(got, ref):
    assert np.array_equal(_counts(got), ref["counts"]), (_counts(got), ref["counts"])
    assert np.array_equal(got["vsd"].view(np.int32), ref["vsd"].view(np.int32))


@gpu
def test_depth_bits_of_a_mixed_object_two_image_call_and_windows():
    """Cube, icosphere and plate under two cameras in ONE call: bit-equal to depth32, window "auto" bit-equal to "full", and in as many
    launch sequences as a small workspace needs."""
    scene, _ = _mixed()
    models = _models(scene)
    P = len(scene["obj_ids"])
    want = np.stack([vo.depth32(scene["objects"][o]["vertices"], scene["objects"][o]["faces"], vo.pose(scene["R_gt"][p], scene["t_gt"][p]),
                                vo.CAMS[scene["image_index"][p]], vo.H, vo.W)[0] for p, o in enumerate(scene["obj_ids"].tolist())])
    args = (models, scene["obj_ids"], scene["R_gt"], scene["t_gt"], scene["K"], (vo.H, vo.W))
    auto = ev.render_depth(*args, image_index=scene["image_index"])
    full = ev.render_depth(*args, image_index=scene["image_index"], window="full")
    split = ev.render_depth(*args, image_index=scene["image_index"], workspace_bytes=40000)
    assert tuple(auto["depth"].shape) == (P, vo.H, vo.W) and auto["depth"].dtype == torch.float32 and (want > 0).sum() > 2000
    for r in (auto, full, split):
        assert np.array_equal(r["depth"].cpu().numpy().view(np.int32), want.view(np.int32)) and r["near_count"] == 0


@gpu
def test_counts_and_errors_equal_the_restatement_and_the_float64_definition():
    """counts equal vsd32 exactly and e bit for bit, for window "auto" and "full".  Against vsd64 on the same float32 depths every count
    differs by at most the fragile pixels of that quantity; the cap on those — at most 1 % of the union for every pair, none at all for at
    least one pair per object — is asserted on the oracle alone."""
    scene, ref = _mixed()
    models = _models(scene)
    frag, union = ref["fragile"], ref["counts"][:, 0]
    assert np.all(union > 0) and np.all(frag.max(axis=1) <= 0.01 * union), (frag.max(axis=1), union)
    for o in (1, 2, 3):
        assert (frag[scene["obj_ids"] == o].max(axis=1) == 0).any(), o
    assert (ref["counts"][:, 1] < union).any() and (ref["counts"][:, 2] > 0).any() and len(np.unique(ref["vsd"])) > 10
    for window in ("auto", "full"):
        got = _run(models, scene, window=window)
        _assert_equals_oracle(got, ref)
        assert got["n_views"] == ref["n_views"] == 2 * len(union) and got["near_count"] == ref["near_count"] == 0
        assert np.all(np.abs(_counts(got) - ref["counts64"]) <= frag)
        clean = frag.max(axis=1) == 0                             # no fragile pixel: equal counts, e differs by its one rounding (e <= 1)
        assert np.all(np.abs(got["vsd"].astype(np.float64) - ref["vsd64"])[clean] <= 2.0 ** -24)
    print("fragile pixels per pair (largest quantity):", frag.max(axis=1).tolist(), "union:", union.tolist())


def _plate_scene():
    cases = vo.plate_cases()
    names = sorted(cases)
    p = vo.plate(vo.PLATE_N)
    scene = {"objects": {3: {"vertices": p["vertices"], "faces": p["faces"], "info": {"diameter": vo.PLATE_DIAMETER}}},
             "obj_ids": np.full(len(names), 3), "image_index": np.arange(len(names), dtype=np.int32), "hw": vo.PLATE_HW,
             "R_est": np.stack([cases[n][0][:3, :3] for n in names]), "t_est": np.stack([cases[n][0][:3, 3] for n in names]),
             "R_gt": np.stack([cases[n][1][:3, :3] for n in names]), "t_gt": np.stack([cases[n][1][:3, 3] for n in names]),
             "depth_mm": np.stack([cases[n][2] for n in names]), "K": vo.k33(np.array([vo.PLATE_K4], dtype=F))[0]}
    return names, cases, scene


@gpu
def test_closed_form_plate_scenes_through_the_kernel():
    names, cases, scene = _plate_scene()
    got = _run(_models(scene), scene)
    for k, n in enumerate(names):
        want = cases[n][3]
        assert got["visib_union"][k] == want["union"] and got["visib_inter"][k] == want["inter"], (n, got["visib_union"][k], got["visib_inter"][k])
        assert np.array_equal(got["vsd"][k], want["e"].astype(F)), (n, got["vsd"][k])
    _assert_equals_oracle(got, vo.reference(scene))


def _edge_scene():
    objs = vo.objects()
    I, rot = np.eye(3), vo.random_rotation(np.random.default_rng(1))
    rows = [(1, rot, (-282.0, 5, 500), (-280.0, 0, 500)), (1, rot, (291.0, 3, 505), (290.0, 0, 500)), (1, rot, (2.0, -214, 495), (0.0, -215, 500)),
            (1, rot, (-3.0, 216, 500), (0.0, 215, 500)),                                                # the four frame borders
            (2, I, (150.0, 0, 500), (-150.0, 0, 500)),                                                   # est and gt windows disjoint
            (1, rot, (2000.0, 0, 500), (2010.0, 0, 500)),                                                # wholly off the frame
            (1, I, (2.0, 1, 32), (0.0, 0, 30)),                                                          # the camera inside the cube: near-dropped
            (2, I, (1.0, 0, 2500), (0.0, 0, 2500)),                                                      # a union under 64 pixels
            (1, rot, (1.0, 2, 303), (0.0, 0, 300))]                                                      # ... and one over 256
    rows += [(2, I, (22.0 + 2 * i, 10, 551 + i), (20.0, 10, 550)) for i in range(8)]                       # eight estimates, one ground truth
    rows.append((2, I, (np.nan, 0, 500), (40.0, -20, 600)))                                              # a NaN pose, last
    depth = np.full((1, vo.H, vo.W), 1500.0, dtype=F)
    depth[0, :, 50:60] = 480.0
    depth[0, 40:50] = 0.0
    return {"objects": objs, "obj_ids": np.array([r[0] for r in rows]), "image_index": np.zeros(len(rows), dtype=np.int32),
            "R_est": np.stack([F(r[1]) for r in rows]), "t_est": np.stack([F(r[2]) for r in rows]), "R_gt": np.stack([F(r[1]) for r in rows]),
            "t_gt": np.stack([F(r[3]) for r in rows]), "depth_mm": depth, "K": vo.k33(vo.CAMS[:1])[0]}


@functools.lru_cache(maxsize=None)
def _edge():
    scene = _edge_scene()
    return scene, vo.reference(scene)


@gpu
def test_edge_shapes_in_one_call():
    scene, ref = _edge()
    models = _models(scene)
    got = _run(models, scene)
    _assert_equals_oracle(got, ref)
    n = len(scene["obj_ids"])
    u = got["visib_union"]
    assert np.all(u[:4] > 0) and u[5] == 0 and np.all(got["vsd"][5] == 1) and 0 < u[7] < 64 and u[8] > 256
    assert got["visib_inter"][4] == 0 and u[4] > 0 and np.all(got["vsd"][4] == 1)                  # disjoint: everything is a miss
    assert got["near_count"] == ref["near_count"] > 0 and got["n_views"] == ref["n_views"] == 2 * 9 + 9 + 2
    assert np.all(got["vsd"][n - 1] == 1) and u[n - 1] > 0                                          # the NaN estimate renders nothing
    # both raster paths in this call: per-lane boxes (<= 64 samples) and tiled ones
    boxes = []
    for p in (8, 9):
        o = int(scene["obj_ids"][p])
        t = ro.Triangles(scene["objects"][o]["vertices"], scene["objects"][o]["faces"], vo.pose(scene["R_gt"][p], scene["t_gt"][p]), tuple(vo.CAMS[0]),
                         vo.H, vo.W, 1.0)
        boxes.append(((t.bx1 - t.bx0 + 1) * (t.by1 - t.by0 + 1))[t.keep])
    assert boxes[0].max() > 64 and boxes[1].max() <= 64
    # the other pairs keep their bits without the NaN pair; P = 1; T = 1 and T = 16; the test depth all missing
    rest = _run(models, scene, rows=np.arange(n - 1))
    for k in KEYS:
        assert np.array_equal(rest[k], got[k][:n - 1]), k
    one = _run(models, scene, rows=np.array([8]))
    assert one["n_views"] == 2 and all(np.array_equal(one[k], got[k][8:9]) for k in KEYS)
    for taus in ([0.2], np.arange(1, 17) / 40.0):
        _assert_equals_oracle(_run(models, scene, taus=taus), vo.reference(scene, taus=taus))
    blind = dict(scene, depth_mm=np.zeros_like(scene["depth_mm"]))
    _assert_equals_oracle(_run(models, blind), vo.reference(blind))


@gpu
def test_one_by_one_and_empty_windows(monkeypatch):
    """Hand-made windows (the planner never makes a 1 x 1 one): a single covered sample, an empty window and a border strip."""
    scene, _ = _edge()
    models = _models(scene)
    rows = np.array([8, 9, 4])
    wins = {8: (60, 44, 61, 45), 9: (0, 0, 0, 0), 4: (0, 30, vo.W, 60)}

    def windows(models_, view_obj, view_img, poses, cams, H, W, near, window):
        out = np.zeros((len(poses), 4), dtype=np.int32)
        for v, P in enumerate(poses):
            p = next(q for q in rows if np.array_equal(vo.pose(scene["R_est"][q], scene["t_est"][q]), P) or
                     np.array_equal(vo.pose(scene["R_gt"][q], scene["t_gt"][q]), P))
            out[v] = wins[int(p)]
        return out

    monkeypatch.setattr(scn, "view_windows", windows)
    got = _run(models, scene, rows=rows)
    for k, p in enumerate(rows.tolist()):
        o = int(scene["obj_ids"][p])
        z = [vo.depth32(scene["objects"][o]["vertices"], scene["objects"][o]["faces"], vo.pose(R, t), vo.CAMS[0], vo.H, vo.W, window=wins[p])[0]
             for R, t in ((scene["R_est"][p], scene["t_est"][p]), (scene["R_gt"][p], scene["t_gt"][p]))]
        c, e = vo.vsd32(z[0], z[1], scene["depth_mm"][0], vo.CAMS[0], scene["objects"][o]["info"]["diameter"])
        assert np.array_equal(_counts(got)[k], c) and np.array_equal(got["vsd"][k], e), (p, _counts(got)[k], c)
    assert got["visib_union"].tolist()[:2] == [1, 0]


@gpu
def test_results_do_not_depend_on_stream_pair_order_or_grouping():
    scene, ref = _mixed()
    models = _models(scene)
    n = len(scene["obj_ids"])
    base = _run(models, scene)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _run(models, scene)
    side.synchronize()
    perm = np.random.default_rng(0).permutation(n)
    shuffled = _run(models, scene, rows=perm)
    single = _run(models, scene, workspace_bytes=1)                # every group holds one pair's two views
    assert base["n_groups"] == 1 and single["n_groups"] == n
    for k in KEYS:
        assert np.array_equal(base[k], other[k]) and np.array_equal(base[k], single[k]) and np.array_equal(base[k][perm], shuffled[k]), k
    _assert_equals_oracle(single, ref)


@gpu
def test_match_and_score_with_depth_equals_the_oracles_recalls_and_ar():
    """Three images of one scene, a cube and a sphere each (the sphere twice in image 1), estimates moved by fixed fractions of the
    diameter: the recalls of all three errors and AR against the plain-container protocol of tests/pose_error_oracle.py fed with the
    oracle's VSD; images_per_call = 2, the callable is asked for exactly the three images."""
    rng = np.random.default_rng(21)
    objs = {o: v for o, v in vo.objects().items() if o != 3}
    for o, v in objs.items():
        v["info"] = dict(v["info"], **({"symmetries_discrete": po.cube_symmetries()} if o == 1 else {}))
    steps = [0.01, 0.04, 0.08, 0.15, 0.3, 0.6]
    est, gts, targets, frames, cams = [], {}, [], {}, {1: {}}
    for im in range(3):
        inst, depth = [], np.full((vo.H, vo.W), 1500.0, dtype=F)
        for o, x in ((1, -120.0), (2, 20.0)) + (((2, 160.0),) if im == 1 else ()):
            R = vo.random_rotation(rng).astype(F).astype(np.float64)
            t = np.array([x, rng.uniform(-60, 60), rng.uniform(450, 600)]).astype(F).astype(np.float64)
            inst.append({"obj": o, "pose": (R, t)})
            d = rng.normal(size=3)
            d *= steps[int(rng.integers(len(steps)))] * objs[o]["info"]["diameter"] / np.linalg.norm(d)
            est.append({"scene": 1, "im": im, "obj": o, "score": float(rng.uniform(0.1, 1)), "pose": (R, (t + d).astype(F).astype(np.float64))})
            z, _ = vo.depth32(objs[o]["vertices"], objs[o]["faces"], vo.pose(R, t), vo.CAMS[im % 2], vo.H, vo.W)
            depth = np.where(z > 0, np.minimum(depth, np.where(z > 0, z, np.inf)), depth)
        gts[(1, im)] = inst
        frames[im] = np.rint(depth).astype(np.uint16)
        cams[1][im] = {"K": vo.k33(vo.CAMS[im % 2:im % 2 + 1])[0].astype(np.float64), "depth_scale": 1.0}
        targets += [(1, im, 1, 1), (1, im, 2, 2 if im == 1 else 1)]
    estimates = {"scene_id": np.ones(len(est), dtype=np.int64), "im_id": np.array([e["im"] for e in est]), "obj_id": np.array([e["obj"] for e in est]),
                 "score": np.array([e["score"] for e in est]), "R": np.array([e["pose"][0] for e in est]), "t": np.array([e["pose"][1] for e in est])}
    gt = {1: {im: {"obj_id": np.array([g["obj"] for g in gts[(1, im)]]), "R": np.array([g["pose"][0] for g in gts[(1, im)]]),
                   "t": np.array([g["pose"][1] for g in gts[(1, im)]])} for im in range(3)}}
    asked = []

    def loader(scene, im):
        asked.append((scene, im))
        return frames[im]

    models = ev.ObjectModels(objs)
    res = ev.match_and_score(estimates, gt, np.array(targets), models, cams, depth_images=loader, images_per_call=2)
    assert sorted(asked) == [(1, 0), (1, 1), (1, 2)] and res["vsd"]["errors"].shape == (len(res["pairs"]["est"]), 10)

    seen = {}

    def e_vsd(k):
        def fn(obj, a, b, scene, im):
            key = (obj, im, vo.pose(*a).tobytes(), vo.pose(*b).tobytes())
            if key not in seen:
                z = [vo.depth32(objs[obj]["vertices"], objs[obj]["faces"], vo.pose(*p), vo.CAMS[im % 2], vo.H, vo.W)[0] for p in (a, b)]
                seen[key] = vo.vsd32(z[0], z[1], frames[im].astype(F), vo.CAMS[im % 2], objs[obj]["info"]["diameter"])[1]
            return float(seen[key][k])
        return fn

    rec = np.stack([po.greedy_recalls(est, gts, targets, e_vsd(k), lambda o, j: (j + 1) / 20.0, 10)[0] for k in range(10)])
    assert np.array_equal(res["recall_vsd"], rec) and rec.min() < rec.max() <= 1 and len(np.unique(rec)) > 2, rec
    assert res["AR_VSD"] == rec.mean() and res["AR"] == (rec.mean() + res["AR_MSSD"] + res["AR_MSPD"]) / 3
    per = np.stack([po.greedy_recalls(est, gts, targets, e_vsd(k), lambda o, j: (j + 1) / 20.0, 10)[1][2] for k in (0, 9)])
    assert np.array_equal(res["per_object"][2]["recall_vsd"][[0, 9]], per)
    plain = ev.match_and_score(estimates, gt, np.array(targets), models, cams)
    assert plain["vsd"] is None and "AR" not in plain and plain["AR_MSSD"] == res["AR_MSSD"] and plain["AR_MSPD"] == res["AR_MSPD"]
