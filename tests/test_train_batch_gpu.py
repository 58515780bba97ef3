"""GPU: the training-pair assembly (csrc/pp_augment.hip via picopose_amd/provider/training_batch.py) bit for bit against the
numpy oracle (tests/train_batch_oracle.py): every augmenter alone, sampled whole programs, the 8-bit resize and normalisation,
whole batches with augmentation off and on; an assembled batch trains; the same seed gives the same batch on any stream."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_batch_oracle as ob  # noqa: E402

from picopose_amd.provider import training_batch as tb  # noqa: E402

gpu = pytest.mark.gpu
H, W = 480, 640


def _frames(rng, n, h=H, w=W):
    """Textured frames: noise over smooth ramps and flat patches (so blends, clips and rounding ties all occur)."""
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.zeros((n, h, w, 4), np.uint8)
    for k in range(n):
        base = (np.sin(yy / rng.uniform(5, 40))[..., None] * rng.uniform(40, 120, 3) + 128 +
                np.cos(xx / rng.uniform(5, 40))[..., None] * rng.uniform(20, 80, 3))
        img = np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255)
        img[h // 3:h // 2, w // 4:w // 3] = rng.integers(0, 256, 3)
        f[k, ..., :3] = img.astype(np.uint8)
        f[k, ..., 3] = rng.integers(0, 2, (h, w)) * rng.choice([1, 255])
    return f


def _boxes(rng):
    """Crop sizes of the spec: 1x1, 3x3, odd, non-square, 480x480, boxes touching the frame border, a few random ones."""
    out = [(0, 1, 0, 1), (5, 8, 7, 10), (H - 37, H, W - 53, W), (0, 480, 160, 640), (100, 101, 639, 640), (0, 57, 0, 91),
           (200, 233, 300, 333), (479, 480, 0, 17), (30, 31, 50, 90)]
    for _ in range(5):
        h, w = rng.integers(2, 150, 2)
        y, x = rng.integers(0, H - h), rng.integers(0, W - w)
        out.append((int(y), int(y + h), int(x), int(x + w)))
    return out


def _devices(frames):
    """The same frames as both kinds of executor input: real (RGB + mask frames) and template (RGBA)."""
    return (torch.from_numpy(np.ascontiguousarray(frames[..., :3])).cuda(), torch.from_numpy(np.ascontiguousarray(frames[..., 3])).cuda(),
            torch.from_numpy(frames).cuda())


def _run(frames, crops, programs):
    """Executor only: frames (n, H, W, 4) uint8, crops [(frame, (y1, y2, x1, x2))] -> the augmented uint8 crops (h, w, 3).
    Even crops read the frames as real views, odd ones as templates."""
    n, h, w = frames.shape[:3]
    plan = tb.plan_augmentation([(k % 2, f * h * w, w, box, 0) for k, (f, box) in enumerate(crops)], programs)
    buf0, buf1, _ = tb.execute_augmentation(*_devices(frames), plan)
    bufs = (buf0.cpu().numpy(), buf1.cpu().numpy())
    out = []
    for d in plan.desc:
        off, ch, cw = int(d[7]), int(d[5]), int(d[6])
        out.append(bufs[(int(d[10]) - 1) & 1][off:off + ch * cw].reshape(ch, cw, 4)[..., :3])
    return out


def _crop(frames, f, box):
    y1, y2, x1, x2 = box
    return np.ascontiguousarray(frames[f, ..., :3][..., ::-1][y1:y2, x1:x2])


def _params(row, rng):
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    return {1: (), 2: (f32(rng.uniform(0, 3)),), 3: (f32(rng.uniform(0, 50)),), 4: (f32(rng.uniform(0.2, 50)),),
            5: (f32(rng.uniform(0.1, 6)),), 6: (f32(rng.uniform(0, 20)),), 7: tuple(int(v) for v in rng.integers(-25, 26, 3)),
            8: tuple(int(v) for v in rng.integers(0, 2, 3)), 9: tuple(f32(v) for v in rng.uniform(0.6, 1.4, 3)),
            10: (f32(rng.uniform(0.6, 1.4)),) * 3, 11: (), 12: tuple(f32(v) for v in rng.uniform(0.5, 2.2, 3)),
            13: (f32(rng.uniform(0, 1)),)}[row]


@gpu
@pytest.mark.parametrize("row", list(range(1, 14)))
def test_each_augmenter_alone(row):
    rng = np.random.default_rng(100 + row)
    frames = _frames(rng, 2)
    boxes = _boxes(rng)
    crops = [(k % 2, b) for k, b in enumerate(boxes)]
    progs = [tb.Program(True, int(rng.integers(0, 2 ** 32)), ((row, _params(row, rng)),)) for _ in crops]
    if row == 2:
        progs[0] = tb.Program(True, 1, ((2, (0.0005,)),))                 # the sigma <= 1e-3 no-op
    got = _run(frames, crops, progs)
    for (f, box), p, g in zip(crops, progs, got):
        src = _crop(frames, f, box)
        ref = ob.run_program(src, p)
        assert np.array_equal(g, ref), (row, box, p, int((g != ref).sum()))
        if row in (3, 4, 5, 6):
            name = ("Sharpness", "Contrast", "Brightness", "Color")[row - 3]
            pil = np.asarray(getattr(ImageEnhance, name)(Image.fromarray(src)).enhance(p.ops[0][1][0]))
            assert np.array_equal(g, pil), (row, box)


@gpu
def test_sampled_whole_programs():
    rng = np.random.default_rng(7)
    frames = _frames(rng, 3)
    aug = tb.ColorAugmentor(np.random.default_rng(8))
    progs = [p for p in aug.sample(320) if p.applied][:224]
    assert len(progs) >= 200 and max(len(tb.pass_starts(p)) for p in progs) == 5   # some take all four passes
    crops = []
    for k in range(len(progs)):
        h, w = (int(v) for v in rng.integers(1, 90, 2)) if k % 7 else (int(rng.integers(150, 300)),) * 2
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        crops.append((k % 3, (y, y + h, x, x + w)))
    got = _run(frames, crops, progs)
    bad = [k for k, ((f, box), p, g) in enumerate(zip(crops, progs, got)) if not np.array_equal(g, ob.run_program(_crop(frames, f, box), p))]
    assert not bad, [(crops[k], progs[k]) for k in bad[:3]]


@gpu
@pytest.mark.parametrize("rgb_mask_flag", [0, 1])
def test_resize_and_normalise(rgb_mask_flag):
    import ctypes

    from picopose_amd import _lib

    rng = np.random.default_rng(3 + rgb_mask_flag)
    frames = _frames(rng, 2)
    boxes = [(0, 448, 0, 448), (10, 458, 100, 548), (0, 224, 0, 224), (5, 305, 7, 307), (40, 77, 3, 40), (0, 1, 0, 1),
             (1, 3, 1, 3), (20, 70, 30, 110), (0, 480, 0, 480), (100, 213, 200, 313), (0, 447, 0, 449), (3, 451, 5, 453)]
    crops = [(k % 2, b) for k, b in enumerate(boxes)]
    S = 224
    alpha = [k % 3 == 0 for k in range(len(crops))]
    plan = tb.plan_augmentation([((k // 2) % 2, f * H * W, W, box, a) for k, ((f, box), a) in enumerate(zip(crops, alpha))],
                                [tb.EMPTY] * len(crops))
    buf0, buf1, d_desc = tb.execute_augmentation(*_devices(frames), plan)
    rgb = torch.empty(len(crops), 3, S, S, device="cuda")
    msk = torch.empty(len(crops), S, S, device="cuda")
    mean, std = (ctypes.c_double * 3)(*ob.CLIP_MEAN), (ctypes.c_double * 3)(*ob.CLIP_STD)
    _lib.check(_lib.lib().pp_augment_resize(buf0.data_ptr(), buf1.data_ptr(), plan.n_buf, d_desc.data_ptr(), len(crops), S,
                                            rgb_mask_flag, mean, std, rgb.data_ptr(), msk.data_ptr(), _lib.stream_ptr()),
               "pp_augment_resize")
    rgb, msk = rgb.cpu().numpy(), msk.cpu().numpy()
    for k, ((f, (y1, y2, x1, x2)), a) in enumerate(zip(crops, alpha)):
        c = _crop(frames, f, (y1, y2, x1, x2))
        m = frames[f, y1:y2, x1:x2, 3]
        if rgb_mask_flag:
            c = c * (m[:, :, None] > 0).astype(np.uint8)
        assert np.array_equal(rgb[k], ob.to_tensor_normalize(ob.resize_linear_u8(c, S))), (k, y2 - y1, x2 - x1)
        mref = (m == 255).astype(int) if a else m.astype(int)
        assert np.array_equal(msk[k], ob.resize_nearest(mref, S).astype(np.float32)), k


def _pair(rng, k):
    """A decoded pair: textured frames, a blob mask in the real frame, an alpha blob in the template, uint16 depths."""
    fr = _frames(rng, 1)[0]
    tf = _frames(rng, 1, 240, 320)[0]
    mask = np.zeros((H, W), np.uint8)
    s = int(rng.integers(12, 200))
    y, x = int(rng.integers(0, H - s)), int(rng.integers(0, W - s))
    mask[y:y + s, x:x + s] = rng.random((s, s)) < 0.7
    alpha = np.zeros((240, 320), np.uint8)
    a = int(rng.integers(10, 200))
    ay, ax = int(rng.integers(0, 240 - a)), int(rng.integers(0, 320 - a))
    alpha[ay:ay + a, ax:ax + a] = rng.choice([0, 100, 255], (a, a), p=[0.1, 0.2, 0.7])
    tf[..., 3] = alpha
    pose = np.eye(4)
    pose[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    pose[:3, 3] = rng.uniform(-3000, 3000, 3)
    if k == 0:                                                         # a 448 x 448 crop: the INTER_AREA switch
        mask[:] = 0
        mask[16:464, 100:548] = 1
    return {"rgb": fr[..., :3], "mask": mask, "depth": rng.integers(0, 65535, (H, W), dtype=np.uint16),
            "depth_scale": float(rng.uniform(0.05, 1.0)), "K": np.array([[572.4114, 0, 325.26], [0, 573.57, 242.05], [0, 0, 1]]),
            "cam_R_m2c": np.linalg.qr(rng.normal(size=(3, 3)))[0].ravel().tolist(), "cam_t_m2c": rng.uniform(-900, 900, 3).tolist(),
            "tem_rgba": tf, "tem_depth": rng.integers(0, 65535, (240, 320), dtype=np.uint16), "tem_pose": pose}


KEYS = [p + k for p in ("real_", "tem_") for k in ("full_depth", "rgb", "bbox", "mask", "M", "K", "pose")]


@gpu
@pytest.mark.parametrize("augment,rgb_mask_flag", [(False, False), (True, False), (True, True)])
def test_assembled_batch_equals_the_oracle(augment, rgb_mask_flag):
    rng = np.random.default_rng(20 + 2 * augment + rgb_mask_flag)
    B = 6
    samples = [_pair(rng, k) for k in range(B)]
    aug = tb.ColorAugmentor(np.random.default_rng(5))
    progs = (aug.sample(B), aug.sample(B)) if augment else ([tb.EMPTY] * B, [tb.EMPTY] * B)
    ep = tb.assemble_training_batch(samples, rgb_mask_flag=rgb_mask_flag, programs=progs)
    ref = ob.collate(samples, *progs, rgb_mask_flag=rgb_mask_flag)
    assert sorted(ep) == sorted(KEYS)
    for k in KEYS:
        got = ep[k].cpu().numpy()
        assert ep[k].dtype == torch.float32 and ep[k].is_cuda and got.shape == ref[k].shape, k
        assert np.array_equal(got, ref[k]), (k, np.abs(got - ref[k]).max())
    assert ep["real_rgb"].shape == (B, 3, 224, 224) and ep["real_full_depth"].shape == (B, H, W)
    assert ep["tem_full_depth"].shape == (B, 240, 320)


@gpu
def test_sampled_batch_is_deterministic_across_calls_and_streams():
    rng = np.random.default_rng(9)
    samples = [_pair(rng, k + 1) for k in range(4)]
    kw = dict(augment_tem=True, size_ratio=1.0)
    a = tb.assemble_training_batch(samples, generator=np.random.default_rng(123), **kw)
    b = tb.assemble_training_batch(samples, generator=np.random.default_rng(123), **kw)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = tb.assemble_training_batch(samples, generator=np.random.default_rng(123), **kw)
    s.synchronize()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    d = tb.assemble_training_batch(samples, generator=np.random.default_rng(124), **kw)
    assert not torch.equal(a["real_rgb"], d["real_rgb"])


def _plane_pair(rng, K, real_pose, tem_pose):
    """A planar textured square (0.3 m, z_obj = 0) rendered into 480 x 640 real and template frames."""
    from netcfg import plane_depth

    out = {}
    for view, pose in (("real", real_pose), ("tem", tem_pose)):
        depth = plane_depth(torch.from_numpy(K).float(), torch.from_numpy(pose).float()).numpy().astype(np.float64)
        v, u = np.mgrid[0:H, 0:W]
        ray = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones((H, W))], -1) * depth[..., None]
        obj = (ray - pose[:3, 3]) @ pose[:3, :3]                       # camera -> object coordinates
        inside = (np.abs(obj[..., 0]) < 0.15) & (np.abs(obj[..., 1]) < 0.15) & (depth > 0)
        tex = np.stack([np.sin(obj[..., 0] * 90) * 100 + 128, np.cos(obj[..., 1] * 70) * 100 + 128,
                        ((np.floor(obj[..., 0] * 40) + np.floor(obj[..., 1] * 40)) % 2) * 200 + 30], -1)
        rgb = np.where(inside[..., None], tex, 20).astype(np.uint8)
        d16 = np.where(inside, np.rint(depth * 10000), 0).astype(np.uint16)
        if view == "real":
            out.update(rgb=rgb, mask=inside.astype(np.uint8), depth=d16, depth_scale=0.1, K=K,
                       cam_R_m2c=pose[:3, :3].ravel().tolist(), cam_t_m2c=(pose[:3, 3] * 1000).tolist())
        else:
            t = pose.copy()
            t[:3, 3] *= 10000.0                                        # template units: t * 0.1 / 1000 = metres
            out.update(tem_rgba=np.concatenate([rgb, (inside * 255).astype(np.uint8)[..., None]], -1), tem_depth=d16, tem_pose=t,
                       templates_K=K)
    return out


@gpu
def test_assembled_batch_trains_at_vit_s():
    from netcfg import euler_pose, small_cfg

    from picopose_amd.picopose import Net
    from picopose_amd.utils.loss_utils import Loss

    rng = np.random.default_rng(31)
    K = np.array([[572.4114, 0, 320], [0, 573.57043, 240], [0, 0, 1.0]])
    samples = []
    for _ in range(2):
        a = (rng.random(6) - 0.5).tolist()
        rp = euler_pose(0.6 * a[0], 0.6 * a[1], 1.2 * a[2], (0.05, -0.03, 0.7)).double().numpy()
        tp = euler_pose(0.6 * a[3], 0.6 * a[4], 1.2 * a[5], (0.0, 0.0, 0.8)).double().numpy()
        samples.append(_plane_pair(rng, K, rp, tp))
    ep = tb.assemble_training_batch(samples, generator=np.random.default_rng(0))
    torch.manual_seed(0)
    net = Net(small_cfg()).cuda().train()
    res = net(ep)
    tot = Loss()(res)
    assert torch.isfinite(tot["loss"]), {k: float(v) for k, v in res.items() if k.startswith("loss")}
    for k, v in res.items():
        if k.startswith("loss"):
            assert torch.isfinite(v).all(), k
    tot["loss"].backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
