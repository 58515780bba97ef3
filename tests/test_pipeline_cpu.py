"""CPU: evaluator-side formatting — no GPU, no library calls."""
import numpy as np

from picopose_amd.pipeline import bop_csv_lines


def test_bop_csv_lines_format_matches_run_test():
    # run_test.py:191-206: scene,img,obj,score,"R (9 values)","t in mm (3 values)",time\n — best hypothesis first
    preds_image = [[{"R_stage_3": np.eye(3).reshape(9), "t_stage_3": np.array([0.01, -0.02, 0.8]) * 1000, "inliers_ratio": 0.9},
                    {"R_stage_3": np.zeros(9), "t_stage_3": np.zeros(3), "inliers_ratio": 0.1}]]
    (line,) = bop_csv_lines(3, 17, [5], [0.75], preds_image, 0.25)
    f = line.split(",")
    assert f[:4] == ["3", "17", "5", "0.75"] and line.endswith("0.25\n")
    assert [float(v) for v in f[4].split(" ")] == list(np.eye(3).reshape(9))
    assert np.allclose([float(v) for v in f[5].split(" ")], [10.0, -20.0, 800.0])


def test_package_seeding_recipe_equals_the_fixture_recipe():
    import torch

    from oracle.weights import seeded_state_dict as ref
    from picopose_amd.utils.seeding import seeded_state_dict as got

    tmpl = {"a.weight": torch.zeros(4, 3, 2, 2), "a.bias": torch.zeros(4), "bn.running_var": torch.zeros(4),
            "bn.running_mean": torch.zeros(4), "bn.num_batches_tracked": torch.zeros((), dtype=torch.long),
            "ls1.gamma": torch.zeros(4), "cls_token": torch.zeros(1, 1, 4), "n.weight": torch.zeros(4)}
    a, b = ref(tmpl, 7), got(tmpl, 7)
    assert all(torch.equal(a[k], b[k]) for k in tmpl)
    # ... and the head calibration (table + application) is the same text on both sides
    from oracle import weights as ow
    from picopose_amd.utils import seeding as ps

    assert ow.HEAD_CALIBRATION == ps.HEAD_CALIBRATION and ow.AFFINE_CALIBRATION == ps.AFFINE_CALIBRATION
    heads = {f"affine_regressor.{h}_predictor.4.{k}": torch.randn(n, 8) if k == "weight" else torch.randn(n)
             for h, n in (("translation", 2), ("scale", 1), ("inplane", 2)) for k in ("weight", "bias")}
    for name in ("flow_pred", "mask_pred"):
        for l in range(3):
            c = 2 if name == "flow_pred" else 1
            heads[f"offset_regressor.flow_decoder.{name}.{l}.predict_layer.weight"] = torch.randn(c, 8, 3, 3)
            heads[f"offset_regressor.flow_decoder.{name}.{l}.predict_layer.bias"] = torch.randn(c)
    cal = dict(ow.HEAD_CALIBRATION["dinov2_vitb14"], affine=ow.AFFINE_CALIBRATION)
    x, y = ow.apply_head_calibration(heads, cal), ps.apply_head_calibration(heads, cal)
    assert all(torch.equal(x[k], y[k]) for k in heads)
    assert not any(torch.equal(x[k], heads[k]) for k in heads if "translation" not in k)


def test_compat_module_name_resolves_like_the_reference_loader():
    """run_test.py:17-20,234-235: `sys.path.append(<model dir>); MODEL = importlib.import_module("picopose")`."""
    import importlib
    import os
    import sys

    import picopose_amd

    sys.path.insert(0, os.path.join(os.path.dirname(picopose_amd.__file__), "compat"))
    try:
        mod = importlib.import_module("picopose")
        from picopose_amd.picopose import Net

        assert mod.Net is Net
    finally:
        sys.path.pop(0)
        sys.modules.pop("picopose", None)


def test_bench_gpus_n_launches_its_own_ranks():
    """`python bench.py --gpus 2` from a plain shell (no WORLD_SIZE) must start two ranks itself (a child
    torch.distributed.run job) — here, without a GPU, both ranks stop at the no-GPU check and say who they are."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PP_BENCH_REHEARSE")}
    import torch

    if torch.cuda.device_count() < 2:
        # more ranks than GPUs, no rehearsal flag: refused with a clear message before anything is launched
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=120)
        assert r.returncode != 0 and "--gpus 2 but this node shows" in r.stdout.decode() and "PP_BENCH_REHEARSE=1" in r.stdout.decode()
        env["PP_BENCH_REHEARSE"] = "1"      # the rehearsal flag lets the launcher start its ranks on fewer GPUs
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode()

    if not torch.cuda.is_available():
        assert r.returncode != 0
        # (the elastic agent stops the surviving rank as soon as the first one has failed, so only one of them is sure
        # to get its message out)
        assert "rank 0 of 2" in out or "rank 1 of 2" in out, out[-1500:]
    # a rank count that contradicts the launcher is refused before any GPU call
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], env=dict(env, WORLD_SIZE="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stdout.decode()


def test_bench_batch_plan_weak_and_strong():
    """bench.py --scaling: weak keeps the workload's crops per rank (global batch x world), strong keeps the GLOBAL batch
    (BASELINE configs[3]: batch 32 sharded 8 ways = 4 crops + 21/20 templates per rank)."""
    import os
    import sys

    import pytest

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from picopose_amd.dist import shard_bounds

    assert bench.batch_plan(32, 8) == (256, 32, "weak")
    assert bench.batch_plan(32, 8, "strong") == (32, 4, "strong")
    assert bench.batch_plan(32, 2, "weak", global_batch=32) == (32, 16, "strong")        # --global-batch implies strong
    assert bench.batch_plan(32, 1, "strong") == (32, 32, "strong")
    assert [shard_bounds(162, 8, r)[1] - shard_bounds(162, 8, r)[0] for r in range(8)] == [21, 21, 20, 20, 20, 20, 20, 20]
    with pytest.raises(SystemExit):
        bench.batch_plan(32, 3, "strong")
    # the SHARDED leg of the default `--gpus N` run (configs[3]: global batch 32, bank cut 21 / 21 / 20 x 6): every rank's plan
    plans = [bench.sharded_leg_plan(32, 162, 8, r) for r in range(8)]
    assert [p[0] for p in plans] == [4] * 8 and [p[2] - p[1] for p in plans] == [21, 21, 20, 20, 20, 20, 20, 20]
    assert plans[0][1] == 0 and plans[-1][2] == 162 and all(plans[r][2] == plans[r + 1][1] for r in range(7))
    assert bench.sharded_leg_plan(32, 162, 2, 1) == (16, 81, 162) and bench.sharded_leg_plan(32, 162, 4, 0) == (8, 0, 41)
    assert bench.sharded_leg_plan(32, 162, 1, 0) is None and bench.sharded_leg_plan(32, 162, 3, 0) is None     # one rank / ranks that do not divide the batch
    # the timed loop alternates two batches only where a look-ahead exists; the extended-bank workload keeps ONE (its cache belongs to it)
    assert bench.input_batches(True, False, False, False) == 2
    assert bench.input_batches(True, False, False, True) == 1 and bench.input_batches(True, False, True, False) == 1
    assert bench.input_batches(False, False, False, False) == 1 and bench.input_batches(True, True, False, False) == 1


def test_compat_import_installs_the_pnp_drop_in(tmp_path):
    """run_test.py:26 does `from utils.pose_recovery import pose_recovery_ransac_pnp` at start-up and imports the model
    module by name only at :234.  With picopose_amd/compat on sys.path that import must re-bind the evaluator's PnP to the
    HIP drop-in — in `utils.pose_recovery` and in the module that already holds the reference function — so that
    run_test.py needs no edit.  Stub `utils` package and stub evaluator module; no GPU."""
    import importlib
    import os
    import sys
    import types

    import picopose_amd
    from picopose_amd.utils.pose_recovery import pose_recovery_ransac_pnp as ours

    pkg = tmp_path / "utils"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "pose_recovery.py").write_text("def pose_recovery_ransac_pnp(*a):\n    return 'reference'\n")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "utils" or k.startswith("utils.") or k == "picopose"}
    sys.path.insert(0, str(tmp_path))
    sys.path.insert(0, os.path.join(os.path.dirname(picopose_amd.__file__), "compat"))
    try:
        evaluator = types.ModuleType("fake_run_test")                 # what run_test.py:26 leaves behind
        exec("from utils.pose_recovery import pose_recovery_ransac_pnp", evaluator.__dict__)
        sys.modules["fake_run_test"] = evaluator
        assert evaluator.pose_recovery_ransac_pnp() == "reference"
        mod = importlib.import_module("picopose")                     # run_test.py:234
        assert evaluator.pose_recovery_ransac_pnp is ours
        assert sys.modules["utils.pose_recovery"].pose_recovery_ransac_pnp is ours
        assert set(mod.installed_in) >= {"utils.pose_recovery", "fake_run_test"}
    finally:
        sys.path.remove(str(tmp_path))
        sys.path.pop(0)
        for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.") or k in ("picopose", "fake_run_test")]:
            sys.modules.pop(k)
        sys.modules.update(saved)


def test_evaluator_loop_reproduces_the_reference_run_test_rows(golden_dir):
    """pipeline.infer_image + bop_csv_lines against tests/golden/run_test_rows.json — the csv rows the
    REFERENCE's own run_test.run_test (run_test.py:100-221) wrote for the same canned case (oracle/gen_golden.py
    gen_run_test): instance mini-batches of `bs`, PnP per (instance, hypothesis), stage-2 fallback (float32, as printed by
    the reference), stable ranking by inlier ratio, best hypothesis per instance, t in millimetres, str() formatting."""
    import json
    import os

    import torch

    from picopose_amd.pipeline import infer_image

    d = json.load(open(os.path.join(golden_dir, "run_test_rows.json")))
    case, hyp = d["case"], d["case"]["hyp"]
    table = {h["uid"]: h for im in case["images"] for inst in im["instances"] for h in inst["hyps"]}

    def net(inputs, hyp_):          # the stub model of the generator: outputs carry only the id of the canned answer
        outs = []
        for tk in range(hyp_):
            uid = inputs["uid"][:, tk]
            outs.append({"pred_tar_pts": uid[:, None, None].repeat(1, 16, 2),
                         "pred_poses": torch.tensor([table[int(u)]["stage2"] for u in uid], dtype=torch.float32)})
        return outs

    def pnp_fn(outputs, real_K):
        H, B = len(outputs), outputs[0]["pred_poses"].shape[0]
        rot, tvec, ratio, ok = np.zeros((H, B, 3, 3)), np.zeros((H, B, 3, 1)), np.zeros((H, B)), np.zeros((H, B), bool)
        for h in range(H):
            for b in range(B):
                e = table[int(outputs[h]["pred_tar_pts"][b, 0, 0])]
                rot[h, b], tvec[h, b, :, 0], ratio[h, b], ok[h, b] = np.array(e["R"]), np.array(e["t"]), e["ratio"], e["ok"]
        return rot, tvec, ratio, ok

    rows = []
    for im in case["images"]:
        inst = im["instances"]
        data = {"score": torch.FloatTensor([[x["score"]] for x in inst])[None], "obj_id": torch.IntTensor([[x["obj_id"]] for x in inst])[None],
                "obj_idx": torch.IntTensor([[x["obj_id"] - 1] for x in inst])[None], "real_K": torch.eye(3).repeat(len(inst), 1, 1)[None],
                "uid": torch.tensor([[h["uid"] for h in x["hyps"]] for x in inst])[None]}
        preds = infer_image(net, data, {}, hyp=hyp, bs=case["bs"], pnp_fn=pnp_fn)
        lines = bop_csv_lines(im["scene_id"], im["img_id"], [data["obj_id"][0][k].item() for k in range(len(inst))],
                              [data["score"][0][k].item() for k in range(len(inst))], preds, 0.0)
        rows += [ln.rsplit(",", 1)[0] for ln in lines]
    assert rows == d["rows"], next((a, b) for a, b in zip(rows, d["rows"]) if a != b)


def test_bench_dump_outputs_writes_float_arrays_within_budget(tmp_path):
    """bench.py --dump-outputs: every array the timed step hands its caller becomes DIR/<name>.npy in float32 / float64 (integers
    exactly); over the byte budget each array is replaced by a seeded sample of its elements, the same one on every run."""
    import os
    import sys

    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    outs = [{"pred_poses": torch.full((2, 4, 4), float(k)), "tem_pose": torch.eye(4).repeat(2, 1, 1), "note": "not an array",
             "pred_tar_pts": torch.arange(-1, 7).reshape(2, 4)} for k in range(3)]
    pnp = (np.zeros((3, 2, 3, 3)), np.ones((3, 2, 3, 1)), np.full((3, 2), 0.5), np.array([[True, False]] * 3))
    arrays = bench.step_outputs("full", (outs, pnp))
    assert sorted(arrays) == ["pnp_inliers_ratio", "pnp_rot", "pnp_success", "pnp_tvec", "pred_poses", "pred_tar_pts", "tem_pose"]
    written = bench.dump_outputs(str(tmp_path / "a"), arrays)
    for name, (shape, sampled) in written.items():
        v = np.load(tmp_path / "a" / (name + ".npy"))
        assert list(v.shape) == shape and not sampled and v.dtype in (np.float32, np.float64), name
    assert np.load(tmp_path / "a" / "pred_poses.npy").shape == (3, 2, 4, 4) and np.load(tmp_path / "a" / "pred_poses.npy")[2].min() == 2
    assert np.load(tmp_path / "a" / "pnp_rot.npy").dtype == np.float64
    assert np.load(tmp_path / "a" / "pnp_success.npy").tolist() == [[1.0, 0.0]] * 3
    pts = np.load(tmp_path / "a" / "pred_tar_pts.npy")
    assert pts.dtype == np.float32 and pts.tolist() == [np.arange(-1, 7).reshape(2, 4).tolist()] * 3      # small integers: float32, exact

    big = {"score": torch.arange(1000, dtype=torch.float32), "index": torch.arange(1000, dtype=torch.int64) + 2 ** 40}
    assert bench.step_outputs("stage1", (big["score"], big["index"])).keys() == big.keys()
    for d in ("b", "c"):
        written = bench.dump_outputs(str(tmp_path / d), big, budget=6000)
        assert all(sampled for _, sampled in written.values())
    sizes = [os.path.getsize(tmp_path / "b" / (n + ".npy")) - 128 for n in big]
    assert sum(sizes) <= 6000, sizes
    for n in big:
        b, c = np.load(tmp_path / "b" / (n + ".npy")), np.load(tmp_path / "c" / (n + ".npy"))
        assert np.array_equal(b, c) and b.size > 0
    idx = np.load(tmp_path / "b" / "index.npy")
    assert idx.dtype == np.float64 and (np.diff(idx) > 0).all() and (idx >= 2 ** 40).all() and (idx == np.round(idx)).all()


def test_bench_refuses_a_run_without_timed_steps():
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stdout.decode(), r.stdout.decode()[-1000:]
