"""CPU: the host layer of picopose_amd/model_info.py and its oracle (tests/model_info_oracle.py): the oracle against closed forms, the
candidate generation, the closure on hand-made groups, every ValueError, the argument checks of the C entries, and the models_info.json
entry through json into symmetry_transforms (the two device calls replaced by the oracle's numpy restatements).  No GPU."""
import ctypes
import json
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_info_oracle as mo  # noqa: E402

from picopose_amd import _lib  # noqa: E402
from picopose_amd import model_info as mi  # noqa: E402  (absent before the feature: every test here fails without it)
from picopose_amd.evaluation import symmetry_transforms  # noqa: E402

F = np.float32


@pytest.fixture
def host_measurements(monkeypatch):
    """The two device calls of model_info.py replaced by the oracle's restatements of the same arithmetic."""
    def diameters(verts, device="cuda"):
        out = []
        for v in verts:
            d2, (i, j) = mo.diameter32(v)
            out.append((float(np.linalg.norm(v[i].astype(np.float64) - v[j].astype(np.float64))), (i, j), d2))
        return out

    def deviations(verts, queries, cand_obj, transforms, symmetric, workspace_bytes=0, device="cuda"):
        T = np.asarray(transforms, dtype=np.float64).reshape(-1, 4, 4)
        out = np.zeros(len(T), dtype=F)
        for o in np.unique(cand_obj):
            rows = np.where(np.asarray(cand_obj) == o)[0]
            out[rows] = mo.symmetric32(verts[o], queries[o], T[rows]) if symmetric else mo.hausdorff32(verts[o], queries[o], mo.map12(T[rows]))
        return out

    monkeypatch.setattr(mi, "_diameters", diameters)
    monkeypatch.setattr(mi, "_deviations", deviations)


# ---- the oracle against closed forms -------------------------------------------------------------------------------------------------
def test_box_diameter_is_its_space_diagonal():
    v = mo.box(20, 30, 50)                                        # lattice coordinates are integers: exact in float32
    want = mo.box_diameter(20, 30, 50)
    assert mo.diameter64(v) == pytest.approx(want, rel=1e-15)
    d2, (i, j) = mo.diameter32(v)
    assert d2 == F(3800) and i < j
    assert np.linalg.norm(v[i].astype(np.float64) - v[j].astype(np.float64)) == pytest.approx(want, rel=1e-15)
    # four space diagonals attain it: the pair is the lexicographically lowest of them
    d = np.linalg.norm(v[:, None].astype(np.float64) - v[None].astype(np.float64), axis=-1)
    ties = sorted((a, b) for a, b in zip(*np.where(np.abs(d - want) < 1e-9)) if a < b)
    assert len(ties) == 4 and (i, j) == ties[0]


@pytest.mark.parametrize("n", [5, 6, 7, 72])
def test_prism_diameter_is_known(n):
    v = mo.prism(n, 30.0, 40.0, mo.SHIFT)
    want = mo.prism_diameter(n, 30.0, 40.0)
    assert abs(mo.diameter64(v) - want) <= 8 * mo.EPS * 60.0      # the float32 rounding of the shifted coordinates (|c| < 64)
    d2, (i, j) = mo.diameter32(v)
    got = float(np.linalg.norm(v[i].astype(np.float64) - v[j].astype(np.float64)))
    assert 0 <= mo.diameter64(v) - got <= mo.DIAMETER_REL * mo.diameter64(v)


def test_diameter32_single_vertex_and_tie_rule():
    assert mo.diameter32(np.zeros((1, 3), dtype=F)) == (F(0), (0, 0))
    v = np.zeros((6, 3), dtype=F)
    v[1], v[2], v[4], v[5] = (1, 0, 0), (-1, 0, 0), (1, 0, 0), (-1, 0, 0)
    assert mo.diameter32(v) == (F(4), (1, 2))


def test_hausdorff_oracles_agree_and_identity_is_zero():
    rng = np.random.default_rng(0)
    full, q = rng.uniform(-50, 50, (300, 3)).astype(F), rng.uniform(-50, 50, (70, 3)).astype(F)
    T = np.stack([np.eye(4), mo.about(np.array([0.0, 0.6, 0.8]), 0.3, np.array([1.0, 2.0, 3.0]))])
    h32, h64 = mo.hausdorff32(full, q, mo.map12(T)), mo.hausdorff64(full, q, mo.map12(T))
    assert np.all(np.abs(h32 - h64) <= mo.hausdorff_bound(q, mo.map12(T), h64))
    assert mo.hausdorff32(full, full[::3], mo.map12(T[:1]))[0] == 0


# ---- candidate generation ------------------------------------------------------------------------------------------------------------
def test_candidate_fractions_count_and_exact_deduplication():
    fr, cont = mi.candidate_fractions()
    totient = lambda n: sum(1 for k in range(1, n + 1) if math.gcd(k, n) == 1)          # noqa: E731
    denominators = {n for n in range(2, 13)} | {d for d in range(2, 73) if 72 % d == 0}
    assert len(fr) == sum(totient(d) for d in denominators) == 95
    assert fr == sorted(set(fr)) and all(0 < f < 1 for f in fr) and len(cont) == 71
    assert fr.count(Fraction(1, 2)) == 1                         # 1/2 = 2/4 = 3/6 = 36/72: once
    assert mi.candidate_fractions(3, 6)[0] == [Fraction(1, 6), Fraction(1, 3), Fraction(1, 2), Fraction(2, 3), Fraction(5, 6)]
    assert (mo.fractions(12, 72)[0], set(mo.fractions(12, 72)[1])) == (fr, cont)


def test_first_round_candidate_count():
    v = mo.box(20, 30, 50, shift=mo.SHIFT, R=mo.generic_rotation())
    seen = []
    res = mi.search_symmetries(v, lambda T: seen.append(len(T)) or np.ones(len(T)), 1e-3)
    assert seen == [6 * 95] and res["candidates"] == 570 and res["symmetries_discrete"] == [] and res["symmetries_continuous"] == []


def test_principal_axes_sign_rule_and_duplicates():
    axes = mi.symmetry_axes(mo.box(20, 30, 50, shift=mo.SHIFT))
    assert np.array_equal(axes, np.eye(3))                       # the box's principal axes ARE the coordinate axes: dropped
    axes = mi.symmetry_axes(mo.box(20, 30, 50, shift=mo.SHIFT, R=mo.generic_rotation()))
    assert axes.shape == (6, 3) and np.allclose(np.linalg.norm(axes, axis=1), 1)
    for a in axes:
        assert a[np.argmax(np.abs(a))] > 0
    R = mo.generic_rotation()
    for col in R.T:                                              # every box axis is among them, up to the sign the rule fixes
        assert min(min(np.abs(a - col).max(), np.abs(a + col).max()) for a in axes[3:]) < 1e-6
    line = np.outer(np.linspace(-1, 1, 50), [-1.0, -0.2, 0.1]).astype(F) + np.random.default_rng(0).normal(0, 1e-3, (50, 3)).astype(F)
    assert mi.symmetry_axes(line)[-1][0] > 0.9                   # the long axis, which eigh may return pointing either way
    assert len(mi.symmetry_axes(line, axes=[[0, 0, 2], [0, 0, -1], [1, 0, 0]])) == 2
    assert [a.tolist() for a in mo.axes_ref(line)] == [a.tolist() for a in mi.symmetry_axes(line)]


# ---- closure on hand-made groups -----------------------------------------------------------------------------------------------------
def _signed_permutation(R):
    return np.abs(np.abs(R) - (np.abs(R) > 0.5)).max() < 1e-9


def _group_measure(member, centre):
    def measure(T):
        return np.array([0.0 if member(t[:3, :3]) and np.abs(t[:3, :3] @ centre + t[:3, 3] - centre).max() < 1e-9 else 1.0 for t in T])
    return measure


def test_closure_builds_the_cube_group_from_its_face_rotations():
    v, c = mo.cube(40, mo.SHIFT), np.array(mo.SHIFT)
    res = mi.search_symmetries(v, _group_measure(_signed_permutation, c), 0.5, axes=np.eye(3))
    R = [np.array(s).reshape(4, 4)[:3, :3] for s in res["symmetries_discrete"]]
    assert len(R) == 23 and all(_signed_permutation(r) and np.linalg.det(r) > 0 for r in R)
    assert len({tuple(np.round(r).astype(int).ravel()) for r in R}) == 23
    first = mi.search_symmetries(v, _group_measure(_signed_permutation, c), 0.5, axes=np.eye(3), max_rounds=0)
    assert len(first["symmetries_discrete"]) == 9                # the 3-fold diagonals and edge 2-folds come only from products
    assert len(mi.search_symmetries(v, _group_measure(_signed_permutation, c), 0.5, axes=np.eye(3), max_elements=12)["symmetries_discrete"]) == 12


def test_closure_d4_and_a_continuous_axis_with_one_flip():
    v, c = mo.cube(40, mo.SHIFT), np.array(mo.SHIFT)
    d4 = lambda R: _signed_permutation(R) and abs(abs(R[2, 2]) - 1) < 1e-9          # noqa: E731
    res = mi.search_symmetries(v, _group_measure(d4, c), 0.5, axes=np.eye(3))
    assert len(res["symmetries_discrete"]) == 7 and res["symmetries_continuous"] == []
    o2 = lambda R: abs(abs(R[2, 2]) - 1) < 1e-9                                     # noqa: E731  every rotation that keeps the z axis
    res = mi.search_symmetries(v, _group_measure(o2, c), 0.5, axes=np.eye(3))
    assert [s["axis"] for s in res["symmetries_continuous"]] == [[0.0, 0.0, 1.0]] and res["symmetries_continuous"][0]["offset"] == list(mo.SHIFT)
    assert len(res["symmetries_discrete"]) == 1                  # the flips about x and y differ by a rotation about z: one is kept
    assert len(res["deviation"]) == 2


@pytest.mark.parametrize("name", list(mo.symmetry_cases()))
def test_reference_rule_counts_and_host_rule_equals_it(name):
    """The expected group sizes of symmetry_cases, confirmed with find_symmetries_ref (the two odd prisms: see the note there), and
    model_info's host rule equal to the restatement, element for element, on the same measurement."""
    v, tol, expected = mo.symmetry_cases()[name]
    ref = mo.find_symmetries_ref(v, tol)
    counts = (len(ref["symmetries_discrete"]), len(ref["symmetries_continuous"]))
    assert counts == expected if expected else counts[0] > 3
    tol_mm = tol if tol != "bop" else mi.bop_tolerance(mo.diameter64(v))
    assert mi.search_symmetries(v, lambda T: mo.symmetric32(v, v, T), tol_mm) == ref
    if name in mo.CENTRED_PRISMS:
        centred = mo.find_symmetries_ref(v, tol, centre=mo.SHIFT)
        assert (len(centred["symmetries_discrete"]), len(centred["symmetries_continuous"])) == mo.CENTRED_PRISMS[name]


# ---- validation: ValueError before any device work -----------------------------------------------------------------------------------
def test_every_value_error():
    v = mo.cube(40)
    bad_vertices = [np.zeros((0, 3), dtype=F), np.zeros((4, 2), dtype=F), np.zeros(3, dtype=F), np.zeros((4, 3), dtype=np.int32),
                    np.array([[0, 0, np.nan]], dtype=F), np.array([[0, np.inf, 0]], dtype=F), np.array([[1e39, 0, 0]])]
    for b in bad_vertices:
        for call in (lambda: mi.model_diameter(b), lambda: mi.symmetry_deviation(b, np.eye(4)[None]), lambda: mi.find_symmetries(b, 1.0),
                     lambda: mi.model_info(b), lambda: mi.models_info({1: v, 2: {"vertices": b}})):
            with pytest.raises(ValueError):
                call()
    shear = np.eye(4)
    shear[0, 1] = 0.1
    scale = np.diag([2.0, 2.0, 2.0, 1.0])
    bottom = np.eye(4)
    bottom[3, 0] = 1.0
    nan = np.eye(4)
    nan[0, 3] = np.nan
    for T in (shear, scale, bottom, nan, np.eye(3), np.zeros((2, 4, 3)), "x"):
        with pytest.raises(ValueError):
            mi.symmetry_deviation(v, T)
    for kw in ({"tol": 0}, {"tol": -1.0}, {"tol": float("nan")}, {"tol": "loose"}, {"tol": None}, {"max_order": 1}, {"continuous_steps": 2},
               {"max_rounds": -1}, {"max_elements": 0}, {"max_points": 0}, {"max_points": 2.5}, {"diameter": -3.0}, {"axes": [[0, 0, 0]]},
               {"axes": [1, 0, 0]}):
        with pytest.raises(ValueError):
            mi.find_symmetries(v, **dict({"tol": 1.0}, **kw))
        with pytest.raises(ValueError):
            mi.model_info(v, "search", **dict({"tol": 1.0}, **kw))
    with pytest.raises(ValueError):
        mi.symmetry_deviation(v, np.eye(4)[None], max_points=-1)
    with pytest.raises(ValueError):
        mi.model_info(v, symmetries="guess")
    with pytest.raises(ValueError):
        mi.model_info(v, tol=1.0)                                # search arguments without a search
    with pytest.raises(ValueError):
        mi.model_info(v, "search", tolerance=1.0)
    with pytest.raises(ValueError):
        mi.model_info(v, {"symmetries_discrete": [shear.reshape(16).tolist()]})
    with pytest.raises(ValueError):
        mi.model_info(v, {"symmetries_discrete": [[1.0] * 15]})
    with pytest.raises(ValueError):
        mi.model_info(v, {"symmetries_continuous": [{"axis": [0, 0, 0], "offset": [0, 0, 0]}]})
    with pytest.raises(ValueError):
        mi.models_info({1: v}, {2: {"symmetries_discrete": []}})
    with pytest.raises(ValueError):
        mi.models_info({})
    with pytest.raises(ValueError):
        mi.search_symmetries(v, lambda T: np.zeros(len(T)), "bop")


def test_c_entries_validate_before_any_device_call():
    L = _lib.lib()
    assert {"pp_model_diameter", "pp_model_diameter_workspace_bytes", "pp_transform_hausdorff",
            "pp_transform_hausdorff_workspace_bytes"} <= set(_lib.declared_symbols())
    need = ctypes.c_size_t()
    off = lambda *a: np.array(a, dtype=np.int32)                  # noqa: E731
    good = off(0, 2049, 5049, 5050)                               # 3, 3 and 1 tiles: 3 * 2 + 3 * 2 + 1 work items
    assert L.pp_model_diameter_workspace_bytes(good.ctypes.data, 3, ctypes.byref(need)) == 0 and need.value == 256 + 256
    for bad in (off(1, 2, 3, 4), off(0, 5, 5, 6), off(0, 5, 4, 6)):
        assert L.pp_model_diameter_workspace_bytes(bad.ctypes.data, 3, ctypes.byref(need)) == -1
    assert L.pp_model_diameter_workspace_bytes(None, 3, ctypes.byref(need)) == -1
    assert L.pp_model_diameter_workspace_bytes(good.ctypes.data, 0, ctypes.byref(need)) == -1
    buf = (ctypes.c_char * 1024)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    assert L.pp_model_diameter(None, p, good.ctypes.data, 3, p, 512, p, p, None) == -1
    assert L.pp_model_diameter(p, p, off(0, 5, 5, 6).ctypes.data, 3, p, 512, p, p, None) == -1
    assert L.pp_model_diameter(p, p, good.ctypes.data, -1, p, 512, p, p, None) == -1
    assert L.pp_model_diameter(p, p, good.ctypes.data, 3, p, 256, p, p, None) == -2           # PP_EWORKSPACE: too small
    assert L.pp_model_diameter(p, p, good.ctypes.data, 3, p + 4, 4096, p, p, None) == -2      # misaligned
    assert L.pp_transform_hausdorff_workspace_bytes(700, 4096, ctypes.byref(need)) == 0 and need.value == 11264          # 700 candidates x 4 tiles x 4 bytes, rounded up to 256
    assert L.pp_transform_hausdorff_workspace_bytes(0, 4096, ctypes.byref(need)) == -1
    assert L.pp_transform_hausdorff_workspace_bytes(1, 0, ctypes.byref(need)) == -1
    assert L.pp_transform_hausdorff_workspace_bytes(1, 65536 * 1024, ctypes.byref(need)) == -1
    cand = off(0, 2, 1)
    call = lambda **kw: L.pp_transform_hausdorff(*[kw.get(k, d) for k, d in (                 # noqa: E731
        ("v", p), ("vo", p), ("q", p), ("qo", p), ("voh", good.ctypes.data), ("qoh", good.ctypes.data), ("n", 3), ("co", p),
        ("coh", cand.ctypes.data), ("T", p), ("C", 3), ("ws", p), ("wsb", 256), ("h", p), ("s", None))])
    assert call(v=None) == -1 and call(T=None) == -1 and call(h=None) == -1 and call(C=-1) == -1 and call(n=0) == -1
    assert call(qoh=off(0, 5, 5, 6).ctypes.data) == -1 and call(voh=off(2, 5, 7, 9).ctypes.data) == -1
    assert call(coh=off(0, 3, 1).ctypes.data) == -1 and call(coh=off(0, -1, 1).ctypes.data) == -1
    assert call(wsb=0) == -2 and call(ws=p + 8) == -2


# ---- the entry ------------------------------------------------------------------------------------------------------------------------
def test_entry_round_trips_through_json_into_symmetry_transforms(host_measurements):
    v = mo.box(20, 30, 50, shift=mo.SHIFT)
    entry = mi.model_info({"vertices": v}, "search", tol=1e-3)
    assert set(entry) == {"diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z", "symmetries_discrete"}
    assert entry["diameter"] == pytest.approx(mo.box_diameter(20, 30, 50), rel=1e-6)
    assert [entry[k] for k in ("min_x", "min_y", "min_z", "size_x", "size_y", "size_z")] == [-3.0, -18.0, -14.0, 20.0, 30.0, 50.0]
    back = json.loads(json.dumps(entry))
    assert back == entry
    S = symmetry_transforms(back)
    assert S.shape == (4, 4, 4) and np.array_equal(S[0], np.eye(4))
    for T in S:                                                   # every one maps the box onto itself, about ITS centre
        moved = v.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        assert np.abs(moved[:, None] - v[None].astype(np.float64)).max(-1).min(axis=1).max() < 1e-4
    plain = mi.model_info(v)
    assert "symmetries_discrete" not in plain and plain["diameter"] == entry["diameter"]
    # a continuous axis and explicit lists
    e72 = mi.model_info(mo.prism(72, 30, 40, mo.SHIFT), "search", tol=1e-3)
    assert len(e72["symmetries_continuous"]) == 1 and len(e72["symmetries_discrete"]) == 1
    assert symmetry_transforms(json.loads(json.dumps(e72))).shape == (2 * 315, 4, 4)
    found = mi.find_symmetries(v, 1e-3)
    assert found == mo.find_symmetries_ref(v, 1e-3)
    explicit = mi.model_info(v, found)
    assert explicit["symmetries_discrete"] == entry["symmetries_discrete"] and "deviation" not in explicit


def test_models_info_batches_and_write_round_trip(host_measurements, tmp_path, monkeypatch):
    meshes = {3: mo.box(20, 30, 50, shift=mo.SHIFT), 11: {"vertices": mo.cube(40, mo.SHIFT)}, 12: mo.prism(72, 30, 40, mo.SHIFT)}
    calls = {"diameter": 0, "deviation": []}
    diam, dev = mi._diameters, mi._deviations
    monkeypatch.setattr(mi, "_diameters", lambda verts, device="cuda": calls.__setitem__("diameter", calls["diameter"] + 1) or diam(verts))
    monkeypatch.setattr(mi, "_deviations", lambda verts, q, obj, T, sym, **kw: calls["deviation"].append(sorted(set(obj.tolist()))) or dev(verts, q, obj, T, sym))
    infos = mi.models_info(meshes, "search", tol=1e-3)
    assert calls["diameter"] == 1 and calls["deviation"][0] == [0, 1, 2]          # one diameter call; the first round of all objects in one
    assert calls["deviation"][1:] == [[1]]                                         # the cube's closure round (the next one has nothing new)
    assert [len(infos[k].get("symmetries_discrete", [])) for k in (3, 11, 12)] == [3, 23, 1]
    for k, v in meshes.items():
        assert infos[k] == mi.model_info(v, "search", tol=1e-3)
    path = tmp_path / "models_info.json"
    mi.write_models_info(path, infos)
    back = json.load(open(path))
    assert back == {str(k): e for k, e in infos.items()}
    assert symmetry_transforms(back["11"]).shape == (24, 4, 4)
