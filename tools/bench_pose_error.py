"""Time pose_errors (picopose_amd/evaluation.py) beside a plain PyTorch formulation on the same GPU and the float64 numpy oracle on the
host.  hipEvents around each call, warm-up first, median, minimum and maximum of the repeats.  The timed region is the whole pose_errors call
as a user makes it: host planning, the upload of the pair table and the workspace allocation included, not the kernels alone, and
the rates derived from it are whole-call rates.  The oracle is imported from tests/ (the package holds no numpy evaluation).

  (a) MSSD + MSPD: --pairs 10000 pairs of a 30 000-vertex object with one continuous symmetry (315 transforms)
  (b) ADD-S:       --adds-pairs 1000 pairs of a 20 000-vertex object

The PyTorch formulation (batched matmul for the transforms, torch.cdist for ADD-S, chunked over pairs to fit memory) and the numpy
oracle are timed on a SUBSAMPLE of the pairs (--torch-pairs, --host-pairs) and extrapolated linearly; the output labels them so.
Prints one JSON line."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_error_oracle as po  # noqa: E402

from picopose_amd import evaluation as ev  # noqa: E402


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [round(min(ms), 3), round(max(ms), 3)]


def poses(rng, n):
    Rg = np.array([po.random_rotation(rng) for _ in range(n)])
    tg = np.stack([rng.uniform(-150, 150, n), rng.uniform(-100, 100, n), rng.uniform(600, 1500, n)], axis=1)
    Re = np.array([R @ po.random_rotation(rng, 0.2) for R in Rg])
    return [a.astype(np.float32) for a in (Re, tg + rng.normal(size=(n, 3)) * 10, Rg, tg)]


def torch_sym(V, sR, st, Re, te, Rg, tg, fx, fy, chunk):
    """MSSD + MSPD with batched matmuls: (chunk, S, Nv, 3) is materialised per chunk."""
    out = []
    sv = torch.einsum("sij,nj->sni", sR, V) + st[:, None]                               # (S, Nv, 3), shared by every pair
    for p0 in range(0, len(Re), chunk):
        e = torch.einsum("pij,nj->pni", Re[p0:p0 + chunk], V) + te[p0:p0 + chunk, None]
        g = torch.einsum("pij,snj->psni", Rg[p0:p0 + chunk], sv) + tg[p0:p0 + chunk, None, None]
        mssd = (e[:, None] - g).norm(dim=-1).amax(dim=2).amin(dim=1)
        pe = torch.stack([fx * e[..., 0], fy * e[..., 1]], dim=-1) / e[..., 2:3]
        pg = torch.stack([fx * g[..., 0], fy * g[..., 1]], dim=-1) / g[..., 2:3]
        out.append((mssd, (pe[:, None] - pg).norm(dim=-1).amax(dim=2).amin(dim=1)))
    return out


def torch_adds(V, Re, te, Rg, tg, chunk):
    out = []
    for p0 in range(0, len(Re), chunk):
        e = torch.einsum("pij,nj->pni", Re[p0:p0 + chunk], V) + te[p0:p0 + chunk, None]
        g = torch.einsum("pij,nj->pni", Rg[p0:p0 + chunk], V) + tg[p0:p0 + chunk, None]
        out.append(torch.cdist(e, g, compute_mode="donot_use_mm_for_euclid_dist").amin(dim=2).mean(dim=1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--vertices", type=int, default=30000)
    ap.add_argument("--adds-pairs", type=int, default=1000)
    ap.add_argument("--adds-vertices", type=int, default=20000)
    ap.add_argument("--torch-pairs", type=int, default=64)
    ap.add_argument("--host-pairs", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    rng = np.random.default_rng(0)
    box = np.array([120.0, 80.0, 60.0])
    objects = {1: {"vertices": (rng.uniform(-1, 1, (a.vertices, 3)) * box).astype(np.float32),
                   "info": {"diameter": 312.4, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}},
               2: {"vertices": (rng.uniform(-1, 1, (a.adds_vertices, 3)) * box).astype(np.float32), "info": {"diameter": 312.4}}}
    models = ev.ObjectModels(objects)
    S = models.n_symmetries(1)
    K = np.array([[1066.778, 0, 312.9869], [0, 1067.487, 241.3109], [0, 0, 1]], dtype=np.float32)
    res = {"pairs": a.pairs, "symmetries": S, "vertices": a.vertices, "adds_pairs": a.adds_pairs, "adds_vertices": a.adds_vertices}

    # (a) MSSD + MSPD
    pa = [torch.from_numpy(x).cuda() for x in poses(rng, a.pairs)]
    ids = np.full(a.pairs, 1)
    for kinds in (("mssd", "mspd"), ("mssd",), ("mspd",)):
        ms, span = timed(lambda: ev.pose_errors(models, ids, *pa, K=K, kinds=kinds, workspace_bytes=1 << 30), a.warmup, a.repeats)
        res["hip_" + "_".join(kinds) + "_ms"] = round(ms, 3)
        res["hip_" + "_".join(kinds) + "_ms_min_max"] = span
    transforms = a.pairs * S * a.vertices
    res["hip_point_transforms_per_s_mssd"] = transforms / (res["hip_mssd_ms"] * 1e-3)
    res["hip_point_transforms_per_s_mspd"] = transforms / (res["hip_mspd_ms"] * 1e-3)
    V = models.vertices[:a.vertices]
    sR, st = models.sym_R[:S].view(S, 3, 3), models.sym_t[:S]
    n = min(a.torch_pairs, a.pairs)
    ms, _ = timed(lambda: torch_sym(V, sR, st, *[x[:n] for x in pa], float(K[0, 0]), float(K[1, 1]), 4), 1, 5)
    res["torch_mssd_mspd_ms_extrapolated"] = round(ms * a.pairs / n, 1)
    res["torch_mssd_mspd_measured_pairs"] = n
    h = min(a.host_pairs, a.pairs)
    T = models.symmetries[0]
    t0 = time.perf_counter()
    for i in range(h):
        po.errors64(objects[1]["vertices"], T, *[x[i].cpu().numpy().astype(np.float64) for x in pa], K.astype(np.float64), kinds=("mssd", "mspd"))
    res["numpy64_mssd_mspd_ms_extrapolated"] = round((time.perf_counter() - t0) * 1e3 * a.pairs / h, 1)
    res["numpy64_measured_pairs"] = h

    # (b) ADD-S
    pb = [torch.from_numpy(x).cuda() for x in poses(rng, a.adds_pairs)]
    ids2 = np.full(a.adds_pairs, 2)
    ms, span = timed(lambda: ev.pose_errors(models, ids2, *pb, kinds=("adds",)), a.warmup, a.repeats)
    res["hip_adds_ms"] = round(ms, 3)
    res["hip_adds_ms_min_max"] = span
    res["hip_adds_point_pairs_per_s"] = a.adds_pairs * a.adds_vertices ** 2 / (ms * 1e-3)
    V2 = models.vertices[a.vertices:]
    n = min(a.torch_pairs, a.adds_pairs)
    ms, _ = timed(lambda: torch_adds(V2, *[x[:n] for x in pb], 2), 1, 5)
    res["torch_adds_ms_extrapolated"] = round(ms * a.adds_pairs / n, 1)
    t0 = time.perf_counter()
    for i in range(h):
        po.errors64(objects[2]["vertices"], np.eye(4)[None], *[x[i].cpu().numpy().astype(np.float64) for x in pb], kinds=("adds",))
    res["numpy64_adds_ms_extrapolated_kdtree"] = round((time.perf_counter() - t0) * 1e3 * a.adds_pairs / h, 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
