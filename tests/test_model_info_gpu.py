"""GPU: csrc/pp_model_info.hip through picopose_amd/model_info.py against tests/model_info_oracle.py: the diameter and its pair equal to
the float32 restatement at the edges of the tiling, within the derived bound of float64, with the tie rule and under a permutation of
the objects; the directed Hausdorff distance equal to its restatement bit for bit, within the derived bound of float64, exactly 0 for
the identity, the same bits under a workspace bound that forces groups, never larger when the query is sub-sampled; find_symmetries equal
to the reference rule element for element on every mesh of the table; and the found symmetries scoring a symmetric estimate."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_info_oracle as mo  # noqa: E402

from picopose_amd import evaluation as ev  # noqa: E402
from picopose_amd import model_info as mi  # noqa: E402  (absent before the feature: every test here fails without it)

gpu = pytest.mark.gpu
F = np.float32
COUNTS = (1, 2, 255, 256, 257, 1023, 1024, 1025)
RAGGED = (2049, 3000, 1)


@functools.lru_cache(maxsize=None)
def _cloud(n, seed=0):
    v = (np.random.default_rng(seed + n).uniform(-1, 1, (n, 3)) * [120.0, 80.0, 60.0]).astype(F)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _diameter_ref(n, seed=0):
    return mo.diameter32(_cloud(n, seed)), mo.diameter64(_cloud(n, seed))


def _check_diameter(v, got, ref32, d64):
    d, pair, d2 = got
    assert (d2, pair) == (ref32[0], tuple(int(k) for k in ref32[1])), (d2, pair, ref32)
    print(f"diameter n={len(v)}: d2max {d2!r} pair {pair} D64 - diameter = {d64 - d:.3e} (bound {mo.DIAMETER_REL * d64:.3e})")
    assert 0 <= d64 - d <= mo.DIAMETER_REL * d64


@gpu
@pytest.mark.parametrize("n", COUNTS)
def test_diameter_equals_the_float32_restatement(n):
    v = _cloud(n)
    ref32, d64 = _diameter_ref(n)
    _check_diameter(v, mi._diameters([v])[0], ref32, d64)
    d, pair = mi.model_diameter(v)
    assert pair == tuple(ref32[1]) and d == float(np.linalg.norm(v[pair[0]].astype(np.float64) - v[pair[1]].astype(np.float64)))


@gpu
def test_diameter_ragged_call_and_object_permutation():
    clouds = [_cloud(n) for n in RAGGED]
    got = mi._diameters(clouds)
    for v, g, n in zip(clouds, got, RAGGED):
        _check_diameter(v, g, *_diameter_ref(n))
    assert got[2][0] == 0.0 and got[2][1] == (0, 0) and got[2][2] == 0
    for perm in ((2, 0, 1), (1, 2, 0)):
        again = mi._diameters([clouds[k] for k in perm])
        assert [again[perm.index(k)] for k in range(3)] == got
    everything = mi._diameters([_cloud(n) for n in COUNTS] + clouds)              # every count in ONE call: the same bits as alone
    assert [e[1:] for e in everything[:len(COUNTS)]] == [(tuple(_diameter_ref(n)[0][1]), _diameter_ref(n)[0][0]) for n in COUNTS]
    assert everything[len(COUNTS):] == got


@gpu
def test_diameter_tie_rule_across_tiles():
    """The maximum is attained by several pairs; the lowest, (5, 1500), straddles two i-tiles; a later pair of the diagonal tile, a pair of
    a later i-tile and a pair found by another workgroup's j-range must not win."""
    v = (np.random.default_rng(1).uniform(-1, 1, (4200, 3))).astype(F)
    v[5] = v[7] = v[2100] = (100, 0, 0)
    v[1500] = v[2050] = v[4100] = (-100, 0, 0)
    got = mi._diameters([v])[0]
    assert got[1:] == ((5, 1500), F(40000)) and mo.diameter32(v) == (F(40000), (5, 1500))
    w = v.copy()
    w[5], w[1500] = v[6], v[1501]                                 # now the lowest is (7, 2050): i in tile 0, j in tile 2 (the second j-range)
    assert mi._diameters([w])[0][1:] == ((7, 2050), F(40000))
    u = v[:1000].copy()
    u[3] = u[200] = (100, 0, 0)
    u[900] = u[990] = (-100, 0, 0)
    u[5] = u[7] = 0
    assert mi._diameters([u])[0][1:] == ((3, 900), F(40000))      # inside the diagonal tile


# ---- Hausdorff -----------------------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (1024, 256), (1025, 257), (300, 2049))           # (query, full)


def _transforms(C, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(C):
        a = rng.normal(size=3)
        out.append(mo.about(a / np.linalg.norm(a), rng.uniform(0, 0.5), rng.uniform(-20, 20, 3)))
        out[-1][:3, 3] += rng.uniform(-5, 5, 3)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _two_objects(sizes, C):
    """Two objects (query, full) of the given sizes and C candidates that alternate between them, with both references."""
    (q0, n0), (q1, n1) = sizes
    verts = [_cloud(n0, 10), _cloud(n1, 20)]
    queries = [_cloud(q0, 30), _cloud(q1, 40)]
    obj = (np.arange(C) % 2).astype(np.int32)
    T12 = mo.map12(_transforms(C, C))
    h32, h64, bound = np.zeros(C, dtype=F), np.zeros(C), np.zeros(C)
    for o in (0, 1):
        rows = np.where(obj == o)[0]
        if len(rows):
            h32[rows] = mo.hausdorff32(verts[o], queries[o], T12[rows])
            h64[rows] = mo.hausdorff64(verts[o], queries[o], T12[rows])
            bound[rows] = mo.hausdorff_bound(queries[o], T12[rows], h64[rows])
    return verts, queries, obj, T12, h32, h64, bound


@gpu
@pytest.mark.parametrize("sizes", [(SIZES[0], SIZES[1]), (SIZES[2], SIZES[3]), (SIZES[3], SIZES[0])])
@pytest.mark.parametrize("C", [1, 37])
def test_hausdorff_equals_the_float32_restatement(sizes, C):
    verts, queries, obj, T12, h32, h64, bound = _two_objects(sizes, C)
    h = mi._hausdorff(verts, queries, obj, T12)
    assert h.dtype == F and np.array_equal(h, h32), np.abs(h - h32).max()
    print(f"hausdorff {sizes} C={C}: max |h - h64| / bound = {(np.abs(h - h64) / bound).max():.3f}, bound <= {bound.max():.3e}")
    assert np.all(np.abs(h.astype(np.float64) - h64) <= bound)


@gpu
def test_hausdorff_groups_under_a_small_workspace_and_candidate_order():
    verts, queries, obj, T12, h32, _, _ = _two_objects((SIZES[2], SIZES[3]), 37)
    assert mi.hausdorff_group_size(37, 1025, 64) == 8             # five calls
    assert np.array_equal(mi._hausdorff(verts, queries, obj, T12, workspace_bytes=64), h32)
    assert np.array_equal(mi._hausdorff(verts, queries, obj, T12, workspace_bytes=1), h32)     # one candidate per call
    perm = np.random.default_rng(0).permutation(37)
    assert np.array_equal(mi._hausdorff(verts, queries, obj[perm], T12[perm]), h32[perm])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = mi._hausdorff(verts[::-1], queries[::-1], 1 - obj, T12)                        # object order, another stream
    assert np.array_equal(other, h32)


@gpu
def test_identity_is_exactly_zero_and_a_subsampled_query_never_exceeds_the_full_one():
    v = _cloud(2100)
    assert mi.symmetry_deviation(v, np.eye(4)[None]).tolist() == [0.0]
    assert mi.symmetry_deviation(v, np.eye(4), max_points=100, symmetric=False).tolist() == [0.0]
    T = _transforms(9, 5)
    full = mi.symmetry_deviation(v, T)
    assert np.array_equal(full, mo.symmetric32(v, v, T))
    for m in (1, 100, 1024, 2099):
        sub = mi.symmetry_deviation(v, T, max_points=m)
        assert np.array_equal(sub, mo.symmetric32(v, mi.subsample(v, m), T)) and np.all(sub <= full)
    one = mi.symmetry_deviation(v, T, symmetric=False)
    assert np.array_equal(one, mo.hausdorff32(v, v, mo.map12(T))) and np.all(one <= full)


# ---- the symmetry search -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _symmetry_ref(name, centred=False):
    v, tol, _ = mo.symmetry_cases()[name]
    return mo.find_symmetries_ref(v, tol, centre=mo.SHIFT if centred else None)


@gpu
@pytest.mark.parametrize("name", list(mo.symmetry_cases()))
def test_find_symmetries_equals_the_reference_rule(name):
    v, tol, expected = mo.symmetry_cases()[name]
    got, ref = mi.find_symmetries(v, tol), _symmetry_ref(name)
    counts = (len(got["symmetries_discrete"]), len(got["symmetries_continuous"]))
    print(f"{name}: {counts} from {got['candidates']} candidates, largest kept deviation {max(got['deviation'] or [0.0]):.3e} mm")
    assert got == ref
    assert counts == expected if expected else counts[0] > 3


@gpu
@pytest.mark.parametrize("name", list(mo.CENTRED_PRISMS))
def test_find_symmetries_of_an_odd_prism_about_its_axis(name):
    """The centre of the vertex box of an odd n-gon is off the prism's axis; with the axis point handed in the dihedral group is found."""
    v, tol, _ = mo.symmetry_cases()[name]
    got = mi.find_symmetries(v, tol, centre=mo.SHIFT)
    assert got == _symmetry_ref(name, True)
    assert (len(got["symmetries_discrete"]), len(got["symmetries_continuous"])) == mo.CENTRED_PRISMS[name]


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_found_symmetries_score_a_symmetric_estimate():
    meshes = {1: mo.box(20, 30, 50, shift=mo.SHIFT), 2: mo.cube(40, mo.SHIFT)}
    infos = mi.models_info(meshes, "search", tol=1e-3)
    assert [len(infos[k]["symmetries_discrete"]) for k in (1, 2)] == [3, 23]
    for k, v in meshes.items():                                   # the batched call is the single calls
        assert infos[k] == mi.model_info(v, "search", tol=1e-3)
        assert infos[k]["diameter"] == mi.model_diameter(v)[0]
    plain = mi.models_info(meshes)
    assert all("symmetries_discrete" not in e for e in plain.values())
    with_sym = ev.ObjectModels({k: {"vertices": v, "info": infos[k]} for k, v in meshes.items()})
    without = ev.ObjectModels({k: {"vertices": v, "info": plain[k]} for k, v in meshes.items()})
    assert [with_sym.n_symmetries(k) for k in (1, 2)] == [4, 24] and [without.n_symmetries(k) for k in (1, 2)] == [1, 1]
    R_gt, t_gt = mo.generic_rotation(), np.array([30.0, -20.0, 250.0])
    ids, Re, te = [], [], []
    for k in (1, 2):
        for s in infos[k]["symmetries_discrete"]:
            S = np.array(s).reshape(4, 4)
            ids.append(k)
            Re.append(R_gt @ S[:3, :3])
            te.append(R_gt @ S[:3, 3] + t_gt)
    n = len(ids)
    args = (np.array(ids), np.array(Re), np.array(te), np.broadcast_to(R_gt, (n, 3, 3)).copy(), np.broadcast_to(t_gt, (n, 3)).copy())
    good = ev.pose_errors(with_sym, *args, kinds=("mssd",))["mssd"].cpu().numpy()
    bad = ev.pose_errors(without, *args, kinds=("mssd",))["mssd"].cpu().numpy()
    print(f"MSSD with the found symmetries <= {good.max():.3e} mm, without >= {bad.min():.3f} mm")
    assert np.all(good < 1e-3) and np.all(bad > 10.0)
