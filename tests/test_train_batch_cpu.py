"""CPU: the training-pair assembly's host side (picopose_amd/provider/training_batch.py) and its numpy oracle
(tests/train_batch_oracle.py) — PIL pins the oracle's enhancers, the sampler's statistics follow the recipe, boxes, M, poses
and depths follow the reference's expressions, bad samples and bad ABI arguments are refused before any device work."""
import os
import sys

import numpy as np
import pytest
from PIL import Image, ImageEnhance

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_batch_oracle as ob  # noqa: E402

from picopose_amd.provider import training_batch as tb  # noqa: E402


@pytest.mark.parametrize("name", ["Sharpness", "Contrast", "Brightness", "Color"])
def test_oracle_enhancers_equal_pil(name):
    fn = {"Sharpness": ob.sharpness, "Contrast": ob.contrast, "Brightness": ob.brightness, "Color": ob.color}[name]
    lo, hi = {"Sharpness": (0, 50), "Contrast": (0.2, 50), "Brightness": (0.1, 6), "Color": (0, 20)}[name]
    rng = np.random.default_rng(1)
    sizes = [(1, 1), (2, 2), (3, 3), (1, 7), (5, 1), (17, 31), (64, 48)] + [tuple(rng.integers(1, 70, 2)) for _ in range(40)]
    for k, (h, w) in enumerate(sizes):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if k % 3 == 0:
            img = (img // 85 * 85).astype(np.uint8)                     # flat regions: the filter's rounding on ties of the blend
        for f in (float(np.float32(rng.uniform(lo, hi))), 1.0, float(np.float32(lo))):
            ref = np.asarray(getattr(ImageEnhance, name)(Image.fromarray(img)).enhance(f))
            assert np.array_equal(fn(img, f), ref), (name, h, w, f)


def test_sampler_statistics():
    n = 20000
    progs = tb.ColorAugmentor(np.random.default_rng(7)).sample(n)
    sd = lambda p, m: 4 * np.sqrt(p * (1 - p) / m)  # noqa: E731
    applied = np.array([p.applied for p in progs])
    assert abs(applied.mean() - 0.8) < sd(0.8, n)
    on = [p for p in progs if p.applied]
    m = len(on)
    fired = np.zeros((m, 14), bool)
    pos = np.zeros((14, 13), np.int64)
    for i, p in enumerate(on):
        rows = [r for r, _ in p.ops]
        assert len(set(rows)) == len(rows)
        fired[i, rows] = True
        # each op's rank among the 13 shuffled augmenters is uniform; its rank among the FIRED ones is what the program
        # shows: compare with the same statistic of the recipe (uniform order restricted to the fired set)
        for k, r in enumerate(rows):
            pos[r, k] += 1
    for r, p in enumerate(tb.GATES, start=1):
        assert abs(fired[:, r].mean() - p) < sd(p, m), (r, fired[:, r].mean(), p)
    # position uniformity: given the fired set of size c, an op sits at each of the c places with probability 1 / c
    cnt = fired[:, 1:].sum(1)
    for r in range(1, 14):
        exp = np.zeros(13)
        for c in range(1, 14):
            exp[:c] += ((cnt == c) & fired[:, r]).sum() / c
        obs = pos[r]
        ok = exp > 0
        assert np.all(np.abs(obs[ok] - exp[ok]) < 4 * np.sqrt(exp[ok]) + 1), (r, obs, exp.round(1))
    par = {r: [prm for p in on for row, prm in p.ops if row == r] for r in range(1, 14)}
    ranges = {2: (0, 3), 3: (0, 50), 4: (0.2, 50), 5: (0.1, 6), 6: (0, 20), 9: (0.6, 1.4), 10: (0.6, 1.4), 12: (0.5, 2.2), 13: (0, 1)}
    for r, (lo, hi) in ranges.items():
        v = np.array(par[r], np.float64).ravel()
        assert v.min() >= np.float32(lo) and v.max() <= np.float32(hi), r
        assert v.min() < lo + 0.05 * (hi - lo) and v.max() > hi - 0.05 * (hi - lo), r
    add = np.array(par[7])
    assert add.min() == -25 and add.max() == 25 and add.dtype.kind == "i"
    for r, p, vals in ((7, 0.3 * (1 - 1 / 51 ** 2), add), (9, 0.5, np.array(par[9])), (12, 0.3, np.array(par[12]))):
        rate = (vals != vals[:, :1]).any(1).mean()
        assert abs(rate - p) < sd(p, len(vals)), (r, rate)
    assert np.all(np.array(par[10])[:, 0] == np.array(par[10])[:, 2])
    inv = np.array(par[8])
    assert abs(inv.mean() - 0.2) < sd(0.2, inv.size)
    assert all(len(p.ops) == 0 for p in progs if not p.applied)
    assert max(len(tb.pass_starts(p)) - 1 for p in progs) <= tb.MAX_PASSES


def test_sampler_determinism_and_record_round_trip():
    a = tb.ColorAugmentor(np.random.default_rng(3)).sample(500)
    b = tb.ColorAugmentor(np.random.default_rng(3)).sample(500)
    assert a == b
    assert a != tb.ColorAugmentor(np.random.default_rng(4)).sample(500)
    heads, ops = tb.program_to_records(a)
    assert heads.dtype == ops.dtype == np.int32 and ops.shape == (500, 13, 8)
    assert tb.records_to_program(heads, ops) == a
    for p, h in zip(a, heads):
        assert h[0] == len(p.ops) and np.uint32(h[1].view(np.uint32)) == p.seed


def test_blur_taps():
    for s in np.float32(np.random.default_rng(0).uniform(0, 3, 200)).tolist() + [1e-4, 1e-3, 0.5, 1.0, 3.0]:
        r, q = tb.gaussian_taps(s)
        _, qo = ob.taps(s)
        assert r == len(qo) // 2 and q[0] + 2 * sum(q[1:]) == 256
        assert list(qo[r:]) == list(q[:r + 1]) and all(v == 0 for v in q[r + 1:])
        assert all(q[i] >= q[i + 1] for i in range(r))


def test_pass_planning():
    prog = tb.Program(True, 5, ((7, (1, 2, 3)), (2, (1.0,)), (13, (0.5,)), (4, (2.0,)), (3, (5.0,)), (1, ())))
    assert tb.pass_starts(prog) == [0, 1, 3, 4, 6]
    crops = [(0, 0, 40, (0, 33, 2, 19), 0), (1, 0, 40, (0, 1, 0, 1), 1)]
    plan = tb.plan_augmentation(crops, [prog, tb.EMPTY])
    assert plan.n_passes == 4 and plan.n_buf == 33 * 17 + 1
    assert list(plan.desc[0, 10:16]) == [4, 0, 1, 3, 4, 6] and list(plan.desc[1, 10:12]) == [1, 0]
    assert list(plan.desc[:, 7]) == [0, 33 * 17]
    t = plan.tiles
    p0 = t[plan.pass_tiles[0]:plan.pass_tiles[1]]
    assert len(p0) == 3 * 2 + 1 and set(map(tuple, p0[:, :3])) >= {(0, 32, 16), (1, 0, 0)}
    for p in range(1, 4):
        assert set(t[plan.pass_tiles[p]:plan.pass_tiles[p + 1], 0]) == {0}


def test_boxes_against_the_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "preprocess_boxes.npz"))
    for m, r, box in zip(z["masks"], z["mask_ratio"], z["mask_boxes"]):
        assert tb.get_bbox(m > 0, float(r)) == list(box) == ob.get_bbox(m > 0, float(r))


def _sample(rng, H=96, W=128, Ht=80, Wt=100):
    mask = np.zeros((H, W), np.uint8)
    y, x = rng.integers(5, H // 2), rng.integers(5, W // 2)
    mask[y:y + rng.integers(10, H // 2), x:x + rng.integers(10, W // 2)] = 1
    rgba = rng.integers(0, 256, (Ht, Wt, 4), dtype=np.uint8)
    rgba[..., 3] = 0
    rgba[10:50, 20:70, 3] = rng.choice([128, 255], (40, 50))
    pose = np.eye(4)
    pose[:3, 3] = rng.uniform(-500, 500, 3)
    return {"rgb": rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "mask": mask,
            "depth": rng.integers(0, 65535, (H, W), dtype=np.uint16), "depth_scale": float(rng.uniform(0.05, 2.0)),
            "K": np.array([[600.0, 0, 64], [0, 601.0, 48], [0, 0, 1]]),
            "cam_R_m2c": list(np.linalg.qr(rng.normal(size=(3, 3)))[0].ravel()), "cam_t_m2c": list(rng.uniform(-900, 900, 3)),
            "tem_rgba": rgba, "tem_depth": rng.integers(0, 65535, (Ht, Wt), dtype=np.uint16), "tem_pose": pose}


def test_host_values_follow_the_reference():
    rng = np.random.default_rng(11)
    for k in range(20):
        s = _sample(rng)
        ratio = 1.0 if k % 2 else float(rng.uniform(1.0, 1.2))
        try:
            hv = tb._prepare(s, ratio, ratio, 224)
        except ValueError:
            continue                                       # a box that leaves the frame at this ratio
        real = ob.process_real(s, None, size_ratio=ratio)
        tem = ob.process_template(s, None, size_ratio=ratio)
        assert hv["bbox"] == real["bbox"] and hv["tem_bbox"] == tem["bbox"]
        for mine, ref in ((hv["M"], real["M"]), (hv["tem_M"], tem["M"]), (hv["pose"], real["pose"]), (hv["tem_pose"], tem["pose"])):
            assert np.array_equal(np.float32(mine), np.float32(ref))
        # the depth kernels' arithmetic (include/picopose_hip.h) against the reference's expressions
        d = s["depth"]
        assert np.array_equal(d.astype(np.float32) * np.float32(s["depth_scale"]) / np.float32(1000), real["full_depth"])
        td = s["tem_depth"]
        assert np.array_equal((td.astype(np.float64) * 0.1 / 1000.0).astype(np.float32), np.float32(tem["full_depth"]))


def test_check_sample_and_value_errors():
    rng = np.random.default_rng(5)
    s = _sample(rng)
    tb.check_sample(s)
    small = dict(s, mask=np.zeros_like(s["mask"]))
    small["mask"][3:8, 3:9] = 1                                          # 30 pixels
    with pytest.raises(ValueError, match="fewer than 32"):
        tb.check_sample(small)
    with pytest.raises(ValueError, match="empty visible mask"):
        tb.check_sample(dict(s, mask=np.zeros_like(s["mask"])))
    empty = s["tem_rgba"].copy()
    empty[..., 3] = 0
    with pytest.raises(ValueError, match="empty template alpha"):
        tb.check_sample(dict(s, tem_rgba=empty))
    with pytest.raises(ValueError, match="match the frame"):
        tb.check_sample(dict(s, depth=s["depth"][:-1]))
    with pytest.raises(ValueError, match="uint16"):
        tb.check_sample(dict(s, tem_depth=s["tem_depth"].astype(np.float32)))
    with pytest.raises(ValueError, match="sample 1: fewer than 32"):
        tb.assemble_training_batch([s, small], device="cpu")
    with pytest.raises(ValueError, match="sample 1: frames must share"):
        tb.assemble_training_batch([s, _sample(rng, H=100)], device="cpu")
    with pytest.raises(ValueError, match="dilate_mask"):
        tb.assemble_training_batch([s], dilate_mask=True)


def test_nearest_template_views():
    rng = np.random.default_rng(2)
    poses = np.tile(np.eye(4), (162, 1, 1))
    poses[:, :3, :3] = np.linalg.qr(rng.normal(size=(162, 3, 3)))[0]
    for _ in range(50):
        R = np.linalg.qr(rng.normal(size=(3, 3)))[0].astype(np.float32).astype(np.float64)
        got = tb.nearest_template_views(R, poses)
        assert np.array_equal(got, ob.sample_template_views(R, poses)) and len(got) == 5
        d = np.linalg.norm(-R[2] - (-poses[:, 2, :3]), axis=1)
        assert d[got].max() <= np.sort(d)[4] + 1e-12


def test_abi_argument_validation_needs_no_gpu():
    import ctypes

    from picopose_amd import _lib

    L = _lib.lib()
    pt = (ctypes.c_int * 5)(0, 1, 1, 1, 1)
    assert L.pp_augment_execute(None, None, 1, None, 1, None, 1, None, 13, None, pt, 1, None, None, 1, None, None) == -1
    fake = 1 << 20                                                       # never dereferenced: validation fails first
    assert L.pp_augment_execute(fake, fake, 1, fake, 1, fake, 1, fake, 13, fake, pt, 5, fake, fake, 1, fake, None) == -1
    assert L.pp_augment_execute(fake, fake, 1, fake, 1, fake, 0, fake, 13, fake, pt, 1, fake, fake, 1, fake, None) == -1
    bad = (ctypes.c_int * 5)(0, 0, 0, 0, 0)
    assert L.pp_augment_execute(fake, fake, 1, fake, 1, fake, 1, fake, 13, fake, bad, 1, fake, fake, 1, fake, None) == -1
    assert L.pp_augment_execute(fake, fake, 1, fake + 1, 1, fake, 1, fake, 13, fake, pt, 1, fake, fake, 1, fake, None) == -1
    m, s = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1)
    assert L.pp_augment_resize(None, None, 1, None, 1, 224, 0, m, s, None, None, None) == -1
    assert L.pp_augment_resize(fake, fake, 1, fake, 1, 0, 0, m, s, fake, fake, None) == -1
    assert L.pp_depth_u16_scaled(None, 10, 1, None, None, None) == -1
    assert L.pp_depth_u16_scaled(fake + 2, 10, 1, fake, fake, None) == -1
    assert L.pp_depth_u16_template(fake, 0, fake, None) == -1
    assert L.pp_depth_u16_template(fake, 10, fake + 4, None) == -1
