"""Model metadata from the mesh alone: what a BOP models_info.json entry holds, computed on the device from the vertices.

    entry = model_info(load_ply(path), symmetries="search")          # {"diameter", "min_x" .., "size_x" .., "symmetries_discrete", ..}
    infos = models_info({obj_id: load_ply(path), ...}, symmetries="search")
    write_models_info("models_info.json", infos)
    models = ObjectModels({obj_id: {"vertices": ..., "faces": ..., "info": infos[obj_id]}, ...})     # evaluation.py, unchanged

BOP's diameter is the largest distance between two vertices (MSSD and VSD thresholds are fractions of it, depth_refine and scene_gt
read it too); it is NOT template_bank.mesh_diameter, the norm of twice the axis-aligned extents that places the template camera.
Both it and a symmetry test are all-pairs problems over the vertices and run in csrc/pp_model_info.hip: the diameter is a maximum over
vertex pairs with its arg-max (pp_model_diameter), a symmetry test is a directed Hausdorff distance, a maximum over vertices of a
nearest-neighbour minimum, for hundreds of candidate transforms at once (pp_transform_hausdorff).  The arithmetic is stated in
include/picopose_hip.h, "MODEL INFO", and restated in numpy by tests/model_info_oracle.py; the kernels equal it bit for bit.

The symmetry search (find_symmetries) is a deterministic rule planned on the host; the kernel only measures.  Its output is a set of
CANDIDATES UNDER A TOLERANCE, in models_info.json's shapes.  Two limits: only rotations are searched, so a mirror symmetry is not
found; and only the geometry is looked at, so a part whose symmetry is broken by its texture is reported symmetric.  It replaces
what the BOP toolkit's calc_models_info.py computes (diameter and bounds); parity with the toolkit is unpinned.  Millimetres."""
import json
import math
from fractions import Fraction

import numpy as np

from . import _lib
from .evaluation import symmetry_transforms

DEFAULT_WORKSPACE_BYTES = 256 << 20
NEAR = 1e-6                                                     # two transforms (axes) closer than this in every entry are one


# ---- validation ----------------------------------------------------------------------------------------------------------------------
def _vertices(mesh_or_vertices, what="vertices"):
    """A mesh dict (template_bank.load_ply's: "vertices", optionally "faces") or an (Nv, 3) float array -> float32 (Nv, 3), contiguous."""
    v = mesh_or_vertices["vertices"] if isinstance(mesh_or_vertices, dict) else mesh_or_vertices
    v = np.asarray(v)
    if v.ndim != 2 or v.shape[1] != 3 or len(v) == 0 or not np.issubdtype(v.dtype, np.floating):
        raise ValueError(f"{what} must be a non-empty (Nv, 3) float array, got {v.dtype} {v.shape}")
    if not np.all(np.isfinite(v)):
        raise ValueError(f"{what} contain a non-finite value")
    with np.errstate(over="ignore"):
        v = np.ascontiguousarray(v, dtype=np.float32)
    if not np.all(np.isfinite(v)):
        raise ValueError(f"{what} overflow float32")
    return v


def _rigid(transforms, what="transforms"):
    """-> (C, 4, 4) float64; ValueError unless every one is finite, ends in the row (0, 0, 0, 1) and has R^T R = I within 1e-6."""
    try:
        T = np.asarray(transforms, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be (C, 4, 4) numbers") from None
    if T.ndim == 2 and T.shape == (4, 4):
        T = T[None]
    if T.ndim != 3 or T.shape[1:] != (4, 4):
        raise ValueError(f"{what} must have shape (C, 4, 4), got {T.shape}")
    if not np.all(np.isfinite(T)):
        raise ValueError(f"{what} hold a non-finite number")
    for k, t in enumerate(T):
        R = t[:3, :3]
        if np.abs(R.T @ R - np.eye(3)).max() > 1e-6 or np.abs(t[3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > 1e-6:
            raise ValueError(f"{what}[{k}] is not a rigid transform (R^T R = I within 1e-6, last row 0 0 0 1)")
    return T


def _check_max_points(max_points):
    if max_points is not None and (not isinstance(max_points, (int, np.integer)) or isinstance(max_points, bool) or max_points <= 0):
        raise ValueError(f"max_points must be None or a positive int, got {max_points!r}")


def _check_search(tol, max_order, continuous_steps, max_rounds, max_elements, diameter):
    if not (tol == "bop" if isinstance(tol, str) else (isinstance(tol, (int, float, np.floating, np.integer)) and not isinstance(tol, bool)
                                                         and math.isfinite(tol) and tol > 0)):
        raise ValueError(f"tol must be 'bop' or a positive number of millimetres, got {tol!r}")
    for name, val, low in (("max_order", max_order, 2), ("continuous_steps", continuous_steps, 3), ("max_rounds", max_rounds, 0),
                           ("max_elements", max_elements, 1)):
        if not isinstance(val, (int, np.integer)) or isinstance(val, bool) or val < low:
            raise ValueError(f"{name} must be an int >= {low}, got {val!r}")
    if diameter is not None and not (isinstance(diameter, (int, float, np.floating, np.integer)) and math.isfinite(diameter) and diameter > 0):
        raise ValueError(f"diameter must be None or a positive number, got {diameter!r}")


def subsample(vertices, max_points):
    """evaluation.ObjectModels' rule: every ceil(Nv / max_points)-th vertex, from the first (all of them for None)."""
    return vertices if max_points is None else np.ascontiguousarray(vertices[::-(-len(vertices) // int(max_points))])


# ---- the device calls ----------------------------------------------------------------------------------------------------------------
def _offsets(parts):
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    if off[-1] >= 2 ** 31:
        raise ValueError("the concatenated models exceed 2^31 rows")
    return off.astype(np.int32)


def _device(device):
    import torch

    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.PicoPoseHipError("picopose_amd runs on the GPU only: model_info needs a CUDA(HIP) device")
    return dev


def _diameters(verts, device="cuda"):
    """ONE pp_model_diameter call over a list of float32 vertex arrays -> [(diameter float64, (i, j), d2max float32), ...]."""
    import torch

    dev = _device(device)
    off = _offsets(verts)
    need = _lib.workspace_bytes("pp_model_diameter_workspace_bytes", off, len(verts))
    with torch.cuda.device(dev):
        v_d, off_d = torch.from_numpy(np.concatenate(verts)).to(dev), torch.from_numpy(off).to(dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        d2 = torch.empty(len(verts), dtype=torch.float32, device=dev)
        pair = torch.empty((len(verts), 2), dtype=torch.int32, device=dev)
        _lib.call("pp_model_diameter", v_d, off_d, off, len(verts), ws, ws.numel(), d2, pair)
        d2, pair = d2.cpu().numpy(), pair.cpu().numpy()
    out = []
    for v, (i, j), d in zip(verts, pair.tolist(), d2):
        out.append((float(np.linalg.norm(v[i].astype(np.float64) - v[j].astype(np.float64))), (int(i), int(j)), d))
    return out


def hausdorff_group_size(n_candidates, max_query_vertices, workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """How many candidates one pp_transform_hausdorff call takes under `workspace_bytes` (at least one)."""
    tiles = -(-int(max_query_vertices) // 1024)
    return int(max(1, min(int(n_candidates), int(workspace_bytes) // (4 * tiles))))


def _hausdorff(verts, queries, cand_obj, T12, workspace_bytes=DEFAULT_WORKSPACE_BYTES, device="cuda"):
    """pp_transform_hausdorff over C candidates of mixed objects, in consecutive groups when the workspace bound asks for it.
    verts / queries: per object float32 (Nv, 3) / (Nq, 3); cand_obj (C,) object index; T12 (C, 12) float32 -> (C,) float32 numpy."""
    import torch

    cand_obj = np.ascontiguousarray(cand_obj, dtype=np.int32)
    T12 = np.ascontiguousarray(T12, dtype=np.float32).reshape(-1, 12)
    C = len(cand_obj)
    if C == 0:
        return np.zeros(0, dtype=np.float32)
    if not (isinstance(workspace_bytes, (int, np.integer)) and workspace_bytes > 0):
        raise ValueError(f"workspace_bytes must be a positive int, got {workspace_bytes!r}")
    dev = _device(device)
    same = all(q is v for q, v in zip(queries, verts))
    v_off, q_off = _offsets(verts), _offsets(queries)
    nq_max = int((q_off[1:] - q_off[:-1])[cand_obj].max())
    group = hausdorff_group_size(C, nq_max, workspace_bytes)
    need = _lib.workspace_bytes("pp_transform_hausdorff_workspace_bytes", group, nq_max)
    with torch.cuda.device(dev):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        v_d, v_off_d = up(np.concatenate(verts)), up(v_off)
        q_d, q_off_d = (v_d, v_off_d) if same else (up(np.concatenate(queries)), up(q_off))
        obj_d, T_d = up(cand_obj), up(T12)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        h = torch.empty(C, dtype=torch.float32, device=dev)
        for c0 in range(0, C, group):
            n = min(group, C - c0)
            _lib.call("pp_transform_hausdorff", v_d, v_off_d, q_d, q_off_d, v_off, q_off, len(verts), obj_d[c0:], cand_obj[c0:], T_d[c0:], n,
                      ws, ws.numel(), h[c0:])
        return h.cpu().numpy()


def map12(T):
    """(C, 4, 4) float64 -> (C, 12) float32 in the kernels' (R row-major, t) layout: every entry rounded once."""
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)
    return np.concatenate([T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]], axis=1).astype(np.float32)


def rigid_inverse(T):
    """(R, t) -> (R^T, -(R^T t)) of one 4 x 4 transform, float64."""
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def _deviations(verts, queries, cand_obj, transforms, symmetric, workspace_bytes=DEFAULT_WORKSPACE_BYTES, device="cuda"):
    """(symmetric) deviations of C float64 transforms of mixed objects in ONE batch: T and, when symmetric, its inverse."""
    T = np.asarray(transforms, dtype=np.float64).reshape(-1, 4, 4)
    cand_obj = np.asarray(cand_obj, dtype=np.int32)
    if not symmetric:
        return _hausdorff(verts, queries, cand_obj, map12(T), workspace_bytes, device)
    both = np.concatenate([T, np.stack([rigid_inverse(t) for t in T])]) if len(T) else T
    h = _hausdorff(verts, queries, np.concatenate([cand_obj, cand_obj]), map12(both), workspace_bytes, device)
    return np.maximum(h[:len(T)], h[len(T):])


# ---- public measurements -------------------------------------------------------------------------------------------------------------
def model_diameter(vertices, device="cuda"):
    """BOP's diameter of one model -> (diameter, (i, j)): the largest distance between two vertices and the vertex pair that attains it.

    The kernel finds the pair in float32 (the lexicographically lowest (i, j) among the pairs whose float32 squared distance is the
    largest); the diameter is the float64 norm of the float64 difference of those two float32 vertices.  Every float32 squared distance is
    within a factor (1 +- 2^-24)^5 of its true value, so with D_true the exact maximum over the float32 vertices:
        0 <= D_true - diameter <= 6 * 2**-24 * D_true.
    One vertex: (0.0, (0, 0)).  ValueError: vertices that are not a non-empty (Nv, 3) float array, or hold a non-finite value."""
    d, pair, _ = _diameters([_vertices(vertices)], device)[0]
    return d, pair


def symmetry_deviation(vertices, transforms, max_points=None, symmetric=True, workspace_bytes=DEFAULT_WORKSPACE_BYTES, device="cuda"):
    """How far each rigid transform is from mapping the vertex set onto itself -> (C,) float32 numpy, millimetres.

    Directed: h(T) = max over x in the query set of min over the vertices y of |T x - y|.  symmetric=True returns max(h(T), h(T^-1)).
    transforms: (C, 4, 4), read as float64 and rounded once to float32 (the inverse is taken in float64 and rounded once).
    max_points sub-samples the QUERY side only, by ObjectModels' every-k-th rule; the y side is always every vertex.  A sub-sampled
    result is therefore a LOWER BOUND of the full one and never an over-estimate: the maximum runs over fewer points, every minimum over
    the same ones.  More candidates than `workspace_bytes` holds partial results for are measured in consecutive groups, same bits.
    ValueError (before any device work): vertices of the wrong shape or not finite, transforms that are not (C, 4, 4) rigid, max_points."""
    v = _vertices(vertices)
    T = _rigid(transforms)
    _check_max_points(max_points)
    q = subsample(v, max_points)
    return _deviations([v], [q], np.zeros(len(T), dtype=np.int32), T, symmetric, workspace_bytes, device)


# ---- the symmetry search: host rule --------------------------------------------------------------------------------------------------
def candidate_fractions(max_order=12, continuous_steps=72):
    """The candidate turns of one axis as exact fractions of a full turn, ascending: k / n for 2 <= n <= max_order, 1 <= k < n, and
    k / continuous_steps for 1 <= k < continuous_steps, each value once.  -> (all fractions, the set of the continuous_steps ones)."""
    cont = {Fraction(k, continuous_steps) for k in range(1, continuous_steps)}
    every = {Fraction(k, n) for n in range(2, max_order + 1) for k in range(1, n)} | cont
    return sorted(every), cont


def _fix_sign(a):
    """The component of largest magnitude (the first on a tie) is made positive."""
    return -a if a[int(np.argmax(np.abs(a)))] < 0 else a


def symmetry_axes(vertices, axes=None):
    """The candidate axes, unit float64 rows: the three coordinate axes, then the three principal axes of the vertex covariance
    (float64 eigh, ascending eigenvalue, sign fixed by the largest component); an axis within 1e-6 of one already listed (or of its
    negative) is dropped.  axes: the caller's own (A, 3) list instead (normalised, the same sign and de-duplication rules)."""
    if axes is None:
        v = np.asarray(vertices, dtype=np.float64)
        d = v - v.mean(axis=0)
        _, vec = np.linalg.eigh(d.T @ d / len(v))
        cand = [np.eye(3)[k] for k in range(3)] + [vec[:, k] for k in range(3)]
    else:
        cand = np.asarray(axes, dtype=np.float64)
        if cand.ndim != 2 or cand.shape[1] != 3 or len(cand) == 0 or not np.all(np.isfinite(cand)) or np.any(np.linalg.norm(cand, axis=1) == 0):
            raise ValueError("axes must be (A, 3) finite non-zero vectors")
        cand = list(cand)
    out = []
    for a in cand:
        a = _fix_sign(a / np.linalg.norm(a))
        if not any(min(np.abs(a - b).max(), np.abs(a + b).max()) <= NEAR for b in out):
            out.append(a)
    return np.stack(out)


def rotation_about(axis, angle, centre):
    """The 4 x 4 rotation by `angle` about the unit `axis` through `centre`: R = c I + s K + (1 - c) a a^T (Rodrigues), t = centre - R centre."""
    x, y, z = (float(c) for c in axis)
    c, s = math.cos(angle), math.sin(angle)
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    a = np.array([x, y, z])
    T = np.eye(4)
    T[:3, :3] = c * np.eye(3) + s * K + (1.0 - c) * np.outer(a, a)
    T[:3, 3] = np.asarray(centre, dtype=np.float64) - T[:3, :3] @ np.asarray(centre, dtype=np.float64)
    return T


def compose(A, B):
    """A B of two 4 x 4 transforms, every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in float64 (a fixed order: the search is deterministic)."""
    out = np.empty((4, 4))
    for r in range(4):
        out[r] = ((A[r, 0] * B[0] + A[r, 1] * B[1]) + A[r, 2] * B[2]) + A[r, 3] * B[3]
    return out


class _Pool:
    """A growing list of 4 x 4 transforms with `near`: is one of them within 1e-6 of T in every entry."""

    def __init__(self):
        self.items, self._flat = [], np.zeros((64, 16))

    def add(self, T):
        if len(self.items) == len(self._flat):
            self._flat = np.concatenate([self._flat, np.zeros_like(self._flat)])
        self._flat[len(self.items)] = T.reshape(16)
        self.items.append(T)

    def near(self, T):
        n = len(self.items)
        return n > 0 and bool((np.abs(self._flat[:n] - T.reshape(16)).max(axis=1) <= NEAR).any())


def _modulo_axes(T, kept, cont_axes, centre):
    """Is T = C E for a rotation C about a continuous axis through the centre and E the identity or a kept element: M = T E^-1 leaves
    the axis direction and the centre where they are, each within 1e-6."""
    for E in [np.eye(4)] + kept:
        M = compose(T, rigid_inverse(E))
        for a in cont_axes:
            if np.abs(M[:3, :3] @ a - a).max() <= NEAR and np.abs(M[:3, :3] @ centre + M[:3, 3] - centre).max() <= NEAR:
                return True
    return False


def _search_steps(v, tol, centre, axes, max_order, continuous_steps, max_rounds, max_elements):
    """The search as a generator: yields (K, 4, 4) float64 transforms to measure, is sent their K symmetric deviations, returns the
    result dict.  One yield for the first round (every axis x every fraction), one per closure round."""
    v64 = v.astype(np.float64)
    centre = (v64.min(axis=0) + v64.max(axis=0)) / 2.0 if centre is None else np.asarray(centre, dtype=np.float64)
    axes = symmetry_axes(v, axes)
    fracs, cont = candidate_fractions(max_order, continuous_steps)
    cands = np.stack([rotation_about(a, 2.0 * math.pi * float(f), centre) for a in axes for f in fracs])
    dev = np.asarray((yield cands), dtype=np.float64).reshape(len(axes), len(fracs))
    measured = len(cands)
    is_cont = [all(dev[a, i] <= tol for i, f in enumerate(fracs) if f in cont) for a in range(len(axes))]
    cont_axes = [axes[a] for a in range(len(axes)) if is_cont[a]]
    cont_dev = [max(float(dev[a, i]) for i, f in enumerate(fracs) if f in cont) for a in range(len(axes)) if is_cont[a]]
    kept, kept_dev, rejected = _Pool(), [], _Pool()
    for a in range(len(axes)):
        if is_cont[a]:
            continue                                             # a continuous axis' own rotations are not listed as discrete
        for i in range(len(fracs)):
            T = cands[a * len(fracs) + i]
            if dev[a, i] > tol:
                rejected.add(T)
            elif len(kept.items) < max_elements and not kept.near(T) and not (cont_axes and _modulo_axes(T, kept.items, cont_axes, centre)):
                kept.add(T)
                kept_dev.append(float(dev[a, i]))
    for _ in range(max_rounds):
        if not kept.items or len(kept.items) >= max_elements:
            break
        new = _Pool()
        for A in list(kept.items):
            for B in list(kept.items):
                T = compose(A, B)
                if np.abs(T - np.eye(4)).max() <= NEAR or kept.near(T) or rejected.near(T) or new.near(T):
                    continue
                if cont_axes and _modulo_axes(T, kept.items, cont_axes, centre):
                    continue
                new.add(T)
        if not new.items:
            break
        d = np.asarray((yield np.stack(new.items)), dtype=np.float64)
        measured += len(new.items)
        added = 0
        for T, e in zip(new.items, d):
            if e > tol:
                rejected.add(T)
            elif len(kept.items) < max_elements and not (cont_axes and _modulo_axes(T, kept.items, cont_axes, centre)):
                kept.add(T)
                kept_dev.append(float(e))
                added += 1
        if not added:
            break
    return {"symmetries_discrete": [T.reshape(16).tolist() for T in kept.items],
            "symmetries_continuous": [{"axis": a.tolist(), "offset": centre.tolist()} for a in cont_axes],
            "candidates": int(measured), "deviation": kept_dev + cont_dev}


def search_symmetries(vertices, measure, tol, centre=None, axes=None, max_order=12, continuous_steps=72, max_rounds=4, max_elements=120):
    """find_symmetries' host rule with the measurement handed in: measure((K, 4, 4) float64 transforms) -> K symmetric deviations (mm).
    tol is a number here.  Needs no device unless `measure` does."""
    _check_search(tol, max_order, continuous_steps, max_rounds, max_elements, None)
    if isinstance(tol, str):
        raise ValueError("search_symmetries takes tol in millimetres")
    gen = _search_steps(_vertices(vertices), float(tol), centre, axes, max_order, continuous_steps, max_rounds, max_elements)
    ask = next(gen)
    while True:
        try:
            ask = gen.send(measure(ask))
        except StopIteration as stop:
            return stop.value


def bop_tolerance(diameter):
    """max(15 mm, 0.1 diameter): the BOP20 paper's rule for POTENTIAL symmetries, written from memory (the paper confirms them by eye)."""
    return max(15.0, 0.1 * float(diameter))


def find_symmetries(vertices, tol="bop", diameter=None, centre=None, axes=None, max_order=12, continuous_steps=72, max_points=4096,
                    max_rounds=4, max_elements=120, device="cuda"):
    """Rotational symmetry CANDIDATES of a model under a tolerance -> {"symmetries_discrete": [16 numbers, row-major 4 x 4, translation
    in millimetres], "symmetries_continuous": [{"axis", "offset"}], "candidates": transforms measured, "deviation": the measured deviation
    (mm) of every discrete entry in order, then the largest one of every continuous entry}, in models_info.json's shapes.

    The rule is deterministic and planned on the host; the device only measures (symmetry_deviation, symmetric):
     1. tol: millimetres, or "bop" = max(15 mm, 0.1 diameter) — the BOP20 paper's rule for POTENTIAL symmetries, written from memory; the
        paper then confirms them by eye, which nothing here does.  `diameter` (else model_diameter's) enters only there.
     2. The centre is the centre of the vertices' axis-aligned box (or `centre`).  The axes are the three coordinate axes and the three
        principal axes of the vertex covariance (symmetry_axes), or `axes`.
     3. Per axis the candidate turns are 2 pi k / n for 2 <= n <= max_order, 1 <= k < n, and 2 pi k / continuous_steps, de-duplicated as
        exact fractions (candidate_fractions); each candidate rotates about the axis through the centre (rotation_about).
     4. An axis whose continuous_steps - 1 rotations all pass is continuous: {"axis", "offset": centre}; its own rotations are not listed.
        Otherwise every passing rotation of the axis is a discrete element.
     5. Closure: the products A B (compose) of kept elements that are new — not the identity, not within 1e-6 of a kept or a rejected
        element, not a kept element (or the identity) times a rotation about a continuous axis through the centre — are measured in one
        more call per round and kept when they pass; until a round adds nothing, or max_rounds or max_elements is reached.
     6. Every measurement is the symmetric deviation max(h(T), h(T^-1)) with the query side sub-sampled to max_points; it passes when it
        is <= tol.  (Sub-sampling can only lower a deviation: see symmetry_deviation.)
    Limits: only rotations are searched, so mirror symmetries are not found; only the geometry is looked at, not the texture.
    ValueError (before any device work): vertices of the wrong shape or not finite, tol not "bop" or positive, max_order < 2,
    continuous_steps < 3, max_rounds < 0, max_elements < 1, max_points, axes."""
    v = _vertices(vertices)
    _check_search(tol, max_order, continuous_steps, max_rounds, max_elements, diameter)
    _check_max_points(max_points)
    if axes is not None:
        symmetry_axes(v, axes)
    if isinstance(tol, str):
        tol = bop_tolerance(diameter if diameter is not None else model_diameter(v, device)[0])
    q = subsample(v, max_points)
    return search_symmetries(v, lambda T: _deviations([v], [q], np.zeros(len(T), dtype=np.int32), T, True, device=device), float(tol),
                             centre, axes, max_order, continuous_steps, max_rounds, max_elements)


# ---- models_info.json ----------------------------------------------------------------------------------------------------------------
def _bounds(v):
    v64 = v.astype(np.float64)
    lo, hi = v64.min(axis=0), v64.max(axis=0)
    return {"min_x": float(lo[0]), "min_y": float(lo[1]), "min_z": float(lo[2]), "size_x": float(hi[0] - lo[0]),
            "size_y": float(hi[1] - lo[1]), "size_z": float(hi[2] - lo[2])}


def _explicit(sym, key):
    """The caller's own symmetry lists -> the two models_info keys, validated (lengths and numbers by symmetry_transforms, rigidity here)."""
    if not isinstance(sym, dict):                                 # (find_symmetries' own result is accepted: its other keys are ignored)
        raise ValueError(f"object {key}: explicit symmetries must be {{'symmetries_discrete': [...], 'symmetries_continuous': [...]}}")
    symmetry_transforms(sym)
    disc = [np.asarray(s, dtype=np.float64).reshape(16).tolist() for s in sym.get("symmetries_discrete", []) or []]
    if disc:
        _rigid(np.array(disc).reshape(-1, 4, 4), f"object {key}: symmetries_discrete")
    cont = [{"axis": np.asarray(s["axis"], dtype=np.float64).tolist(), "offset": np.asarray(s["offset"], dtype=np.float64).tolist()}
            for s in sym.get("symmetries_continuous", []) or []]
    return {"symmetries_discrete": disc, "symmetries_continuous": cont}


def models_info(meshes, symmetries=None, device="cuda", **search):
    """{obj_id: mesh or vertices} -> {obj_id: models_info.json entry}: "diameter", "min_x/y/z", "size_x/y/z" (float64 min / max of the
    float32 vertices on the host) and, when asked for, "symmetries_discrete" / "symmetries_continuous" (empty lists are left out).

    symmetries: None (none), "search" (find_symmetries per object, **search its keyword arguments; the result's "candidates" and
    "deviation" are not part of the entry), or {obj_id: {"symmetries_discrete": [...], "symmetries_continuous": [...]}} the caller's own
    lists for some or all objects (validated: rigid, the shapes symmetry_transforms reads).  ONE diameter call covers all objects, and
    every round of the search is ONE Hausdorff call over the candidates of all objects (the first round holds nearly all of them).
    The entries feed ObjectModels({id: {"vertices", "faces", "info": entry}}) and symmetry_transforms(entry) unchanged."""
    if not isinstance(meshes, dict) or not meshes:
        raise ValueError("meshes must be a non-empty {obj_id: mesh or vertices} dict")
    keys = list(meshes)
    verts = [_vertices(meshes[k], f"object {k}: vertices") for k in keys]
    explicit = {}
    if isinstance(symmetries, dict):
        unknown = [k for k in symmetries if k not in meshes]
        if unknown:
            raise ValueError(f"symmetries names unknown objects {unknown}")
        explicit = {k: _explicit(s, k) for k, s in symmetries.items()}
    elif symmetries not in (None, "search"):
        raise ValueError(f"symmetries must be None, 'search' or a dict of explicit lists, got {symmetries!r}")
    elif symmetries is None and search:
        raise ValueError(f"search arguments {sorted(search)} without symmetries='search'")
    if symmetries == "search":
        opts = dict(tol="bop", diameter=None, centre=None, axes=None, max_order=12, continuous_steps=72, max_points=4096, max_rounds=4,
                    max_elements=120)
        extra = set(search) - set(opts)
        if extra:
            raise ValueError(f"unknown search arguments {sorted(extra)}")
        opts.update(search)
        _check_search(opts["tol"], opts["max_order"], opts["continuous_steps"], opts["max_rounds"], opts["max_elements"], opts["diameter"])
        _check_max_points(opts["max_points"])
        for v in verts:
            if opts["axes"] is not None:
                symmetry_axes(v, opts["axes"])
    diam = _diameters(verts, device)
    out = {}
    for k, v, (d, _, _) in zip(keys, verts, diam):
        out[k] = dict({"diameter": d}, **_bounds(v))
        for name, val in explicit.get(k, {}).items():
            if val:
                out[k][name] = val
    if symmetries == "search":
        queries = [subsample(v, opts["max_points"]) for v in verts]
        gens, asks, found = [], {}, {}
        for n, (v, (d, _, _)) in enumerate(zip(verts, diam)):
            tol = bop_tolerance(opts["diameter"] if opts["diameter"] is not None else d) if isinstance(opts["tol"], str) else float(opts["tol"])
            gens.append(_search_steps(v, tol, opts["centre"], opts["axes"], opts["max_order"], opts["continuous_steps"], opts["max_rounds"],
                                      opts["max_elements"]))
            asks[n] = next(gens[n])
        while asks:
            order = sorted(asks)
            dev = _deviations(verts, queries, np.concatenate([np.full(len(asks[n]), n, dtype=np.int32) for n in order]),
                              np.concatenate([asks[n] for n in order]), True, device=device)
            at = 0
            for n in order:
                mine, at = dev[at:at + len(asks[n])], at + len(asks[n])
                try:
                    asks[n] = gens[n].send(mine)
                except StopIteration as stop:
                    found[n] = stop.value
                    del asks[n]
        for n, k in enumerate(keys):
            for name in ("symmetries_discrete", "symmetries_continuous"):
                if found[n][name]:
                    out[k][name] = found[n][name]
    return out


def model_info(mesh_or_vertices, symmetries=None, device="cuda", **search):
    """One models_info.json entry of one model: models_info for a single object.  symmetries: None, "search" (**search: find_symmetries'
    keyword arguments) or the explicit {"symmetries_discrete": [...], "symmetries_continuous": [...]}."""
    sym = {0: symmetries} if isinstance(symmetries, dict) else symmetries
    return models_info({0: mesh_or_vertices}, sym, device, **search)[0]


def write_models_info(path, infos):
    """Write {obj_id: entry} as models_info.json (string keys, as BOP's files have them)."""
    with open(path, "w") as fh:
        json.dump({str(k): v for k, v in infos.items()}, fh, indent=2)
