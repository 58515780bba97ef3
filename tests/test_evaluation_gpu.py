"""GPU: pp_pose_errors (picopose_amd/evaluation.py) against tests/pose_error_oracle.py: MSSD, MSPD and their symmetry indices bit-equal
to the float32 restatement, every error inside its float32 bound of the float64 definitions, determinism across streams, pair order
and chunking, the localization recalls equal to the oracle's, and onboard -> infer -> results rows -> scores end to end."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_error_oracle as po  # noqa: E402
import render_oracle as ro  # noqa: E402

from picopose_amd import evaluation as ev  # noqa: E402

gpu = pytest.mark.gpu
ALL = ("mssd", "mspd", "add", "adds")


def _syms(models, obj_id):
    """The float32 symmetry transforms the device holds for an object: (sym_R (S, 9), sym_t (S, 3), the same as (S, 4, 4) float64)."""
    k = models.index[int(obj_id)]
    s0, s1 = models.sym_off[k], models.sym_off[k + 1]
    T = np.tile(np.eye(4), (s1 - s0, 1, 1))
    T[:, :3, :3], T[:, :3, 3] = models.sym_R_host[s0:s1].reshape(-1, 3, 3), models.sym_t_host[s0:s1]
    return models.sym_R_host[s0:s1], models.sym_t_host[s0:s1], T


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items() if isinstance(v, torch.Tensor)}


@gpu
def test_mixed_call_equals_the_restatement_and_the_definitions():
    """256 pairs mixing a cube (24 symmetries), a 10 242-vertex sphere (315) and a 30 000-vertex random mesh (1) in ONE call, estimates at
    1 mm / 1 degree and at 100 mm / up to 90 degrees."""
    objects, pairs = po.mixed_inputs()
    models = ev.ObjectModels(objects)
    assert [models.n_symmetries(o) for o in (1, 2, 3)] == [24, 315, 1]
    got = _host(ev.pose_errors(models, pairs["obj_ids"], pairs["R_est"], pairs["t_est"], pairs["R_gt"], pairs["t_gt"], K=pairs["K"], kinds=ALL))
    assert len(pairs["obj_ids"]) >= 256 and set(pairs["obj_ids"].tolist()) == {1, 2, 3}
    worst = {k: 0.0 for k in ALL + ("add32", "adds32")}
    for i, o in enumerate(pairs["obj_ids"].tolist()):
        sR, st, T = _syms(models, o)
        V = objects[o]["vertices"]
        a = [pairs[n][i] for n in ("R_est", "t_est", "R_gt", "t_gt")]
        Kp = pairs["K"][i].astype(np.float64)
        e32 = po.errors32(V, sR, st, *a, pairs["K"][i][0, 0], pairs["K"][i][1, 1])
        e64 = po.errors64(V, T, *[x.astype(np.float64) for x in a], Kp)
        for k in ("mssd", "mspd"):
            assert got[k][i].view(np.int32) == np.float32(e32[k]).view(np.int32), (k, i, o, got[k][i], e32[k])
            assert got[k + "_sym"][i] == e32[k + "_sym"], (k, i, o)
        b = po.metric_bound(po.max_norm(V, T), a[1], a[3])
        bp = po.mspd_bound(po.max_norm(V, T), a[1], a[3], max(Kp[0, 0], Kp[1, 1]), po.min_depth(V, T, *[x.astype(np.float64) for x in a]))
        for k in ("add", "adds"):
            worst[k + "32"] = max(worst[k + "32"], abs(float(got[k][i]) - float(e32[k])) / b)
            assert abs(float(got[k][i]) - float(e32[k])) <= b, (k, i, o, got[k][i], e32[k], b)
        for k in ALL:
            lim = bp if k == "mspd" else b
            worst[k] = max(worst[k], abs(float(got[k][i]) - e64[k]) / lim)
            assert abs(float(got[k][i]) - e64[k]) <= lim, (k, i, o, got[k][i], e64[k], lim)
    print("largest error / bound:", {k: round(v, 4) for k, v in worst.items()})


@gpu
def test_adds_at_the_tile_edges_equals_the_restatement_and_the_definition():
    """ADD-S vertex counts around the 256-point LDS tile and the 1024-point workgroup tile (one point, the last lane clamped, a full
    tile, one point into the next tile), three pairs per count in ONE call, held to what the mixed call holds ADD-S to."""
    counts = (1, 255, 256, 257, 1023, 1024, 1025, 2049)
    rng = np.random.default_rng(11)
    objects = {o: {"vertices": (rng.uniform(-1, 1, (n, 3)) * [120.0, 80.0, 60.0]).astype(np.float32), "info": {"diameter": 312.4}}
               for o, n in enumerate(counts, start=1)}
    _, pairs = po.mixed_inputs(seed=7, n_pairs=3 * len(counts))  # the poses only: near and far estimates alternate
    ids = np.repeat(np.arange(1, len(counts) + 1), 3)
    models = ev.ObjectModels(objects)
    got = _host(ev.pose_errors(models, ids, pairs["R_est"], pairs["t_est"], pairs["R_gt"], pairs["t_gt"], kinds=("adds",)))
    for i, o in enumerate(ids.tolist()):
        sR, st, T = _syms(models, o)
        V = objects[o]["vertices"]
        a = [pairs[n][i] for n in ("R_est", "t_est", "R_gt", "t_gt")]
        e32 = po.errors32(V, sR, st, *a, kinds=("adds",))
        e64 = po.errors64(V, T, *[x.astype(np.float64) for x in a], kinds=("adds",))
        b = po.metric_bound(po.max_norm(V, T), a[1], a[3])
        print(len(V), i, "adds", got["adds"][i], "restatement", e32["adds"], "definition", e64["adds"], "bound", b)
        assert abs(float(got["adds"][i]) - float(e32["adds"])) <= b, (len(V), i, got["adds"][i], e32["adds"], b)
        assert abs(float(got["adds"][i]) - e64["adds"]) <= b, (len(V), i, got["adds"][i], e64["adds"], b)


@gpu
def test_a_pair_behind_the_camera_has_infinite_mspd():
    objects, pairs = po.mixed_inputs(seed=5, n_pairs=64)
    models = ev.ObjectModels(objects)
    te, tg = pairs["t_est"].copy(), pairs["t_gt"].copy()
    te[3, 2], tg[10, 2] = -800.0, 0.0                            # an estimate behind the camera; a ground truth that straddles its plane
    got = _host(ev.pose_errors(models, pairs["obj_ids"], pairs["R_est"], te, pairs["R_gt"], tg, K=pairs["K"], kinds=("mssd", "mspd")))
    assert got["mspd"][3] == np.inf and got["mspd"][10] == np.inf and got["mspd_sym"][3] == 0
    rest = np.delete(np.arange(64), [3, 10])
    assert np.all(np.isfinite(got["mspd"][rest])) and np.all(np.isfinite(got["mssd"]))


@gpu
def test_a_non_finite_pose_is_infinitely_wrong_never_perfect():
    """A NaN or an infinity in a pose must not be dropped by the running maximum: MSSD and MSPD are +inf (as the restatement says), ADD
    and ADD-S are not finite, and the other pairs of the call keep their bits."""
    objects, pairs = po.mixed_inputs(seed=5, n_pairs=64)
    models = ev.ObjectModels(objects)
    args = {n: pairs[n].copy() for n in ("R_est", "t_est", "R_gt", "t_gt")}
    clean = _host(ev.pose_errors(models, pairs["obj_ids"], *args.values(), K=pairs["K"], kinds=ALL))
    bad = {}
    for o in (1, 2, 3):                                           # per object: a NaN in t_est, a NaN in R_gt, an infinity in R_est
        rows = np.where(pairs["obj_ids"] == o)[0]
        args["t_est"][rows[0], 1] = np.nan
        args["R_gt"][rows[1], 2, 0] = np.nan
        args["R_est"][rows[2], 0, 0] = np.inf
        bad.update({int(r): o for r in rows[:3]})
    got = _host(ev.pose_errors(models, pairs["obj_ids"], *args.values(), K=pairs["K"], kinds=ALL))
    for i, o in bad.items():
        assert got["mssd"][i] == np.inf and got["mspd"][i] == np.inf, (i, o, got["mssd"][i], got["mspd"][i])
        assert not np.isfinite(got["add"][i]) and not np.isfinite(got["adds"][i]), (i, o, got["add"][i], got["adds"][i])
        sR, st, _T = _syms(models, o)
        e32 = po.errors32(objects[o]["vertices"], sR, st, *[args[n][i] for n in args], pairs["K"][i][0, 0], pairs["K"][i][1, 1], kinds=("mssd", "mspd"))
        assert e32["mssd"] == np.inf and e32["mspd"] == np.inf and got["mssd_sym"][i] == e32["mssd_sym"] and got["mspd_sym"][i] == e32["mspd_sym"]
    rest = np.array([i for i in range(64) if i not in bad])
    for k in clean:
        assert np.array_equal(got[k][rest].view(np.int32), clean[k][rest].view(np.int32)), k


@gpu
def test_match_and_score_never_matches_a_non_finite_estimate():
    """Two instances, inst_count 2: the best-scored estimate holds a NaN (what str(nan) in a results row parses to), the other is exact.
    Half the targets are matched at every threshold of both errors; before the NaN rule the NaN estimate scored MSSD 0."""
    V = (np.random.default_rng(0).uniform(-1, 1, (300, 3)) * 40).astype(np.float32)
    models = ev.ObjectModels({7: {"vertices": V, "info": {"diameter": 120.0}}})
    Rg = np.array([po.random_rotation(np.random.default_rng(k)) for k in (1, 2)])
    tg = np.array([[-150.0, 0, 800], [150.0, 20, 900]])
    lines = ["1,4,7,0.9," + " ".join(str(v) for v in Rg[0].ravel()) + ",nan 0.0 800.0,0.1\n",
             "1,4,7,0.5," + " ".join(str(v) for v in Rg[1].ravel()) + "," + " ".join(str(v) for v in tg[1]) + ",0.1\n"]
    est = ev.read_bop_results(lines)
    assert np.isnan(est["t"][0, 0])
    gt = {1: {4: {"obj_id": np.array([7, 7]), "R": Rg, "t": tg}}}
    cams = {1: {4: {"K": np.array([[600.0, 0, 320], [0, 600.0, 240], [0, 0, 1]]), "depth_scale": 1.0}}}
    res = ev.match_and_score(est, gt, np.array([[1, 4, 7, 2]]), models, cams)
    assert res["recall_mssd"].tolist() == [0.5] * 10 and res["recall_mspd"].tolist() == [0.5] * 10
    from_nan = res["pairs"]["est"] == 0
    assert np.all(res["pairs"]["mssd"][from_nan] == np.inf) and np.all(res["pairs"]["mspd"][from_nan] == np.inf)
    with pytest.raises(ValueError, match="scene 1, image 4"):
        ev.match_and_score(est, gt, np.array([[1, 4, 7, 2]]), models, {1: {}})
    lists = ev.pose_errors(models, [7], Rg[:1].tolist(), tg[:1].tolist(), Rg[:1].tolist(), tg[:1].tolist(), K=cams[1][4]["K"].tolist())
    assert float(lists["mssd"][0]) == 0.0 and float(lists["mspd"][0]) == 0.0          # nested lists, as json.load gives them


@gpu
def test_results_do_not_depend_on_stream_pair_order_or_chunking():
    objects, pairs = po.mixed_inputs(seed=7, n_pairs=64)
    models = ev.ObjectModels(objects)
    args = [pairs[n] for n in ("obj_ids", "R_est", "t_est", "R_gt", "t_gt")]
    base = ev.pose_errors(models, *args, K=pairs["K"], kinds=ALL)
    torch.cuda.synchronize()
    keys = [k for k, v in base.items() if isinstance(v, torch.Tensor)]
    assert sorted(keys) == sorted(ALL + ("mssd_sym", "mspd_sym"))
    again = ev.pose_errors(models, *args, K=pairs["K"], kinds=ALL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ev.pose_errors(models, *args, K=pairs["K"], kinds=ALL)
    side.synchronize()
    perm = np.random.default_rng(0).permutation(64)
    shuffled = ev.pose_errors(models, *[a[perm] for a in args], K=pairs["K"][perm], kinds=ALL)
    per_pair = 315 * 56 + 30 * 8 + 1024                          # composed maps + per-symmetry errors + ADD-S tiles of one pair
    chunked = ev.pose_errors(models, *args, K=pairs["K"], kinds=ALL, workspace_bytes=20 * per_pair)     # 64 pairs in >= 3 pieces
    assert ev.pose_error_chunks(models, pairs["obj_ids"], ALL, workspace_bytes=20 * per_pair) >= 3      # from the library's own workspace query
    assert ev.pose_error_chunks(models, pairs["obj_ids"], ALL) == 1
    torch.cuda.synchronize()
    inv = torch.from_numpy(np.argsort(perm)).cuda()
    for k in keys:
        assert torch.equal(base[k], again[k]) and torch.equal(base[k], other[k]) and torch.equal(base[k], chunked[k]), k
        assert torch.equal(base[k], shuffled[k][inv]), k
    one = ev.pose_errors(models, *args, kinds=("add",))           # a single kind, no K
    assert torch.equal(one["add"], base["add"]) and set(one) == {"add"}
    sub = ev.ObjectModels(objects, max_points=1000)
    r = ev.pose_errors(sub, *args, kinds=("adds", "add"))
    assert r["adds_max_points"] == 1000 and torch.equal(r["add"], base["add"])
    i = int(np.where(pairs["obj_ids"] == 3)[0][0])
    V = objects[3]["vertices"]
    want = po.errors64(V, np.eye(4)[None], *[pairs[n][i].astype(np.float64) for n in ("R_est", "t_est", "R_gt", "t_gt")], kinds=("adds",),
                       V_adds=V[::30])
    assert abs(float(r["adds"][i]) - want["adds"]) <= po.metric_bound(po.max_norm(V, np.eye(4)[None]), pairs["t_est"][i], pairs["t_gt"][i])


def _synthetic_set(rng):
    """2 scenes x 20 images, 3 objects; per image object 3 once and objects 1 and 2 once or twice (instances 400 mm apart); every estimate
    is its ground truth moved by m x diameter, m from a fixed list, along a random direction, with a small rotation for objects 1, 2."""
    cube = ro.cube(40.0)["vertices"]
    objects = {1: {"vertices": cube, "info": {"diameter": 80.0 * math.sqrt(3.0), "symmetries_discrete": po.cube_symmetries()}},
               2: {"vertices": ro.icosphere(2, 50.0)["vertices"],
                   "info": {"diameter": 100.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}},
               3: {"vertices": (rng.uniform(-1, 1, (500, 3)) * [60.0, 40.0, 30.0]).astype(np.float32), "info": {"diameter": 150.0}}}
    steps = [0.02, 0.07, 0.12, 0.22, 0.33, 0.47, 0.62, 0.9]
    est, gt, cams, targets, moves3 = [], {}, {}, [], []
    for scene in (1, 2):
        gt[scene], cams[scene] = {}, {}
        for im in range(20):
            K = np.array([[1066.778, 0, 312.9869], [0, 1067.487, 241.3109], [0, 0, 1]]) if scene == 1 else \
                np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.049], [0, 0, 1]])
            cams[scene][im] = {"K": K, "depth_scale": 1.0}
            inst = []
            for obj in (1, 2, 3):
                count = 1 if obj == 3 else 1 + (im + obj) % 2
                for c in range(count):
                    R = po.random_rotation(rng).astype(np.float32).astype(np.float64)
                    t = np.array([-200.0 + 400.0 * c + rng.uniform(-20, 20), rng.uniform(-100, 100), rng.uniform(700, 1400)]).astype(np.float32)
                    inst.append((obj, R, t.astype(np.float64)))
                    m = steps[int(rng.integers(len(steps)))]
                    d = rng.normal(size=3)
                    d *= m * objects[obj]["info"]["diameter"] / np.linalg.norm(d)
                    Re = R if obj == 3 else R @ po.random_rotation(rng, 0.02)
                    est.append({"scene": scene, "im": im, "obj": obj, "score": float(rng.uniform(0.1, 1.0)),
                                "pose": (Re.astype(np.float32).astype(np.float64), (t + d).astype(np.float32).astype(np.float64))})
                    if obj == 3:
                        moves3.append(np.linalg.norm(est[-1]["pose"][1] - t.astype(np.float64)) / 150.0)
                targets.append((scene, im, obj, count))
            gt[scene][im] = {"obj_id": np.array([i[0] for i in inst]), "R": np.array([i[1] for i in inst]), "t": np.array([i[2] for i in inst])}
    order = rng.permutation(len(est))
    return objects, [est[i] for i in order], gt, cams, targets, np.array(moves3)


@gpu
def test_match_and_score_equals_the_oracles_recalls():
    objects, est, gt, cams, targets, moves3 = _synthetic_set(np.random.default_rng(11))
    assert sum(len(gt[s]) for s in gt) >= 40
    models = ev.ObjectModels(objects)
    estimates = {"scene_id": np.array([e["scene"] for e in est]), "im_id": np.array([e["im"] for e in est]),
                 "obj_id": np.array([e["obj"] for e in est]), "score": np.array([e["score"] for e in est]),
                 "R": np.array([e["pose"][0] for e in est]), "t": np.array([e["pose"][1] for e in est])}
    res = ev.match_and_score(estimates, gt, np.array(targets), models, cams, image_width=640)
    gts = {(s, im): [{"obj": int(o), "pose": (R, t)} for o, R, t in zip(g["obj_id"], g["R"], g["t"])] for s in gt for im, g in gt[s].items()}
    diam = {o: objects[o]["info"]["diameter"] for o in objects}
    bounds = {"mssd": [], "mspd": []}

    def err(kind):
        def fn(obj, a, b, scene, im):
            T = _syms(models, obj)[2]
            V = objects[obj]["vertices"]
            e = po.errors64(V, T, *a, *b, cams[scene][im]["K"], kinds=(kind,))[kind]
            bounds[kind].append(po.metric_bound(po.max_norm(V, T), a[1], b[1]) if kind == "mssd" else
                                po.mspd_bound(po.max_norm(V, T), a[1], b[1], cams[scene][im]["K"][1, 1], po.min_depth(V, T, *a, *b)))
            return e
        return fn

    want = {}
    for kind, limit in (("mssd", lambda o, k: diam[o] * ((k + 1) / 20.0)), ("mspd", lambda o, k: 5.0 * (k + 1))):
        rec, per_obj, seen = po.greedy_recalls(est, gts, targets, err(kind), limit, 10)
        # a recall can only flip where an error lies within the float32 bound of a limit: none of the oracle's does
        lims = np.array([[limit(o, k) for k in range(10)] for o in (1, 2, 3)]).ravel()
        gap = np.abs(seen[:, None] - lims[None]).min(axis=1)
        assert np.all(gap > np.array(bounds[kind])), (kind, gap.min())
        want[kind] = (rec, per_obj)
        assert np.array_equal(res["recall_" + kind], rec), (kind, res["recall_" + kind], rec)
        for o in (1, 2, 3):
            assert np.array_equal(res["per_object"][o]["recall_" + kind], per_obj[o]), (kind, o)
    assert res["AR_MSSD"] == want["mssd"][0].mean() and res["AR_MSPD"] == want["mspd"][0].mean() and res["vsd"] is None
    # known in advance: object 3 has no symmetry, one instance per image and purely translated estimates, so MSSD = the move
    known = np.array([(moves3 < (k + 1) / 20.0).mean() for k in range(10)])
    assert np.array_equal(res["per_object"][3]["recall_mssd"], known) and 0 < known[0] < known[-1] < 1
    assert res["n_targets"] == sum(t[3] for t in targets) and len(res["pairs"]["mssd"]) == len(res["pairs"]["est"])


@gpu
def test_onboard_infer_write_read_score_end_to_end(golden_dir, monkeypatch):
    """The poses infer_image returns for two generated objects, written with bop_csv_lines, read back and scored against the poses the
    query views were rendered with.  Random weights: the errors are large and say nothing about accuracy; this checks that the round trip
    loses nothing, that the errors are finite and that they equal the oracle."""
    from netcfg import small_cfg
    from oracle.weights import seeded_state_dict
    from picopose_amd import ops
    from picopose_amd.picopose import Net
    from picopose_amd.pipeline import bop_csv_lines, infer_image
    from picopose_amd.provider import template_bank as tb
    from picopose_amd.utils.preprocess import crop_instance

    monkeypatch.setattr(ops, "SATURATION_FLAG", False)
    net = Net(small_cfg())
    net.load_state_dict(seeded_state_dict(net.state_dict(), 5))
    net = net.cuda().eval()
    meshes = [ro.cube(40.0), ro.icosphere(3, 50.0)]
    views = np.load(os.path.join(golden_dir, "template_view_poses_level1.npy"))[::9]
    bank = tb.onboard_objects(net, meshes, views, bs=7)
    rng = np.random.default_rng(9)
    inst, obj_idx, truth = [], [], []
    for o, m in enumerate(meshes):
        for _ in range(2):
            q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
            P = np.eye(4)
            P[:3, :3] = q * np.sign(np.linalg.det(q))
            P[:3, 3] = [rng.uniform(-60, 60), rng.uniform(-40, 40), rng.uniform(450, 650)]
            rgba = tb.render_views(m, P[None])["rgba"][0].cpu().numpy()
            mask = (rgba[..., 3] > 0).astype(np.uint8)
            ys, xs = np.where(mask)
            inst.append(crop_instance(rgba[..., :3], mask, [int(xs.min()), int(ys.min()), int(np.ptp(xs)) + 1, int(np.ptp(ys)) + 1]))
            obj_idx.append(o)
            truth.append(P)
    data = {"real_rgb": torch.stack([i["rgb"] for i in inst])[None], "real_mask": torch.stack([i["mask"] for i in inst])[None],
            "real_M": torch.stack([i["M"] for i in inst])[None].cuda(), "real_pts2d": torch.stack([i["pts2d"] for i in inst])[None].float().cuda(),
            "real_K": torch.from_numpy(tb.TEMPLATE_K).float()[None, None].repeat(1, 4, 1, 1).cuda(),
            "real_pose": torch.eye(4)[None, None].repeat(1, 4, 1, 1).cuda(),
            "obj_idx": torch.tensor([obj_idx], device="cuda"), "score": torch.ones(1, 4, device="cuda")}
    preds = infer_image(net, data, bank, hyp=2, bs=3, indexed_bank=True)
    obj_ids = [o + 1 for o in obj_idx]
    lines = bop_csv_lines(1, 0, obj_ids, [1.0, 0.9, 0.8, 0.7], preds, 0.5)
    rows = ev.read_bop_results(lines)
    for k, p in enumerate(preds):                                # the parsed rows equal the written poses to the digits str() printed
        assert rows["R"][k].ravel().tolist() == [float(str(v)) for v in p[0]["R_stage_3"]]
        assert rows["t"][k].tolist() == [float(str(v)) for v in p[0]["t_stage_3"]]
    objects = {1: {"vertices": meshes[0]["vertices"], "info": {"diameter": 80.0 * math.sqrt(3.0), "symmetries_discrete": po.cube_symmetries()}},
               2: {"vertices": meshes[1]["vertices"], "info": {"diameter": 100.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}}
    models = ev.ObjectModels(objects)
    Rg, tg = np.array([P[:3, :3] for P in truth]), np.array([P[:3, 3] for P in truth])
    got = _host(ev.pose_errors(models, rows["obj_id"], rows["R"], rows["t"], Rg, tg, K=tb.TEMPLATE_K, kinds=ALL))
    Kf = tb.TEMPLATE_K.astype(np.float32)
    for i, o in enumerate(obj_ids):
        sR, st, T = _syms(models, o)
        a = [x.astype(np.float32) for x in (rows["R"][i], rows["t"][i], Rg[i], tg[i])]
        e32 = po.errors32(objects[o]["vertices"], sR, st, *a, Kf[0, 0], Kf[1, 1])
        e64 = po.errors64(objects[o]["vertices"], T, *[x.astype(np.float64) for x in a], tb.TEMPLATE_K)
        b = po.metric_bound(po.max_norm(objects[o]["vertices"], T), a[1], a[3])
        for k in ALL:
            assert np.isfinite(got[k][i]) or (k == "mspd" and e32[k] == np.inf), (k, i)
        for k in ("mssd", "mspd"):
            assert got[k][i].view(np.int32) == np.float32(e32[k]).view(np.int32) and got[k + "_sym"][i] == e32[k + "_sym"], (k, i)
        for k in ("mssd", "add", "adds"):
            assert abs(float(got[k][i]) - e64[k]) <= b, (k, i, got[k][i], e64[k], b)
    print("end-to-end errors (random weights, no accuracy claim):", {k: got[k].round(2).tolist() for k in ALL})
