"""Scoring poses against ground truth on the device: the BOP pose errors MSSD and MSPD (Hodan et al., "BOP Challenge 2020 on 6D
Object Localization", section 2.2), ADD and ADD-S (Hinterstoisser et al. 2012), and the BOP localization recall on top of them.

    models = ObjectModels({obj_id: {"vertices": load_ply(path)["vertices"], "info": models_info[str(obj_id)]}, ...})
    err = pose_errors(models, obj_ids, R_est, t_est, R_gt, t_gt, K=K)            # {"mssd", "mspd", "mssd_sym", "mspd_sym"}
    res = match_and_score(read_bop_results(csv), {scene: read_scene_gt(...)}, read_targets(...), models,
                          {scene: read_scene_camera(...)})                        # {"AR_MSSD", "AR_MSPD", "vsd": None, ...}
    vsd = vsd_errors(models, obj_ids, R_est, t_est, R_gt, t_gt, K, depth_u16, depth_scale=1.0)   # needs "faces" in the models
    res = match_and_score(..., depth_images=lambda scene, im: depth_png_as_array)  # adds "AR_VSD" and "AR" = the three-term mean

For an estimate (R^, t^), a ground truth (R_, t_), the model vertices V (millimetres), the object's symmetry set S and the camera K:

    MSSD  = min over S of max over x in V of |(R^ x + t^) - (R_ (S x) + t_)|                    (mm)
    MSPD  = min over S of max over x in V of |proj_K(R^ x + t^) - proj_K(R_ (S x) + t_)|        (px)
    ADD   = mean over x of |(R^ x + t^) - (R_ x + t_)|
    ADD-S = mean over x of min over y in V of |(R^ x + t^) - (R_ y + t_)|

The arithmetic of the kernels (float32, stated operation by operation in include/picopose_hip.h) is restated in numpy by
tests/pose_error_oracle.py.  Translations are millimetres everywhere, as the results rows (pipeline.bop_csv_lines) and scene_gt.json
hold them.

VSD, the third term of the BOP average recall, needs the test depth images and two depth renders per pair, so it has its own entry
point: vsd_errors renders every distinct (image, object, pose) view once into a ragged z-buffer (a host-planned window per view)
and reduces every pair on the device (csrc/pp_vsd.hip; the definition and the arithmetic are stated in include/picopose_hip.h and
restated by tests/vsd_oracle.py; the windows, the view groups and the packing of a call's tables into the PpScene of the ABI are
scene.py's, shared with depth_refine.py and scene_gt.py).  It is the BOP toolkit's VSD (visib_mode "bop19", step cost) written from memory: parity with
the toolkit's pixels is unpinned, and a triangle that reaches the near plane is dropped whole where the toolkit's renderer clips it.
match_and_score computes it when it is given the depth images, and then also returns AR = (AR_VSD + AR_MSSD + AR_MSPD) / 3."""
import json
import math
import os

import numpy as np
import torch

from . import _lib
from . import scene as scn
from .scene import DEFAULT_WORKSPACE_BYTES, plan_window  # noqa: F401  (documented names of this module)

KINDS = {"mssd": _lib.PP_EVAL_MSSD, "mspd": _lib.PP_EVAL_MSPD, "add": _lib.PP_EVAL_ADD, "adds": _lib.PP_EVAL_ADDS}
MSSD_THRESHOLDS = np.arange(1, 11) / 20.0                       # 0.05 .. 0.5 of the object diameter
MSPD_THRESHOLDS = np.arange(1, 11) * 5.0                        # 5 r .. 50 r pixels, r = image_width / 640
VSD_TAUS = np.arange(1, 11) / 20.0                              # misalignment tolerances, 0.05 .. 0.5 of the object diameter
VSD_THRESHOLDS = np.arange(1, 11) / 20.0                        # a pair is correct at (tau, theta) when e_tau < theta
VSD_MAX_TAUS = _lib.PP_VSD_MAX_TAUS


def _rotation(axis, angle):
    """Rodrigues' formula for a unit axis."""
    x, y, z = axis
    c, s = math.cos(angle), math.sin(angle)
    k = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return c * np.eye(3) + s * k + (1.0 - c) * np.outer(axis, axis)


def symmetry_transforms(model_info, max_sym_disc_step=0.01):
    """The symmetry set of one entry of a BOP models_info.json -> (S, 4, 4) float64, identity first.

    `symmetries_discrete`: lists of 16 numbers, a row-major 4 x 4 rigid transform with its translation in millimetres; the discrete
    set is the identity followed by the listed transforms.  `symmetries_continuous`: {"axis", "offset"} entries; each is discretised
    by the BOP toolkit's rule into n = ceil(pi / max_sym_disc_step) rotations by k 2 pi / n, k = 0 .. n - 1, about `axis` through
    `offset` (R = rot(axis, angle), t = offset - R offset); 0.01 gives 315.  Without a continuous symmetry the result is the
    discrete set; with one it is every product continuous x discrete, T = T_cont T_disc, ordered discrete-major (so row 0 is the
    identity), duplicates kept.  Several continuous entries contribute their rotations to one list; they are not multiplied with
    each other.  ValueError: an entry of the wrong length, a zero axis, a non-finite number, a step that is not positive."""
    if not isinstance(model_info, dict):
        raise ValueError("model_info must be one entry (a dict) of models_info.json")
    if not (isinstance(max_sym_disc_step, (int, float)) and math.isfinite(max_sym_disc_step) and max_sym_disc_step > 0):
        raise ValueError(f"max_sym_disc_step must be a positive number, got {max_sym_disc_step!r}")
    disc = [np.eye(4)]
    for k, sym in enumerate(model_info.get("symmetries_discrete", []) or []):
        a = np.asarray(sym, dtype=np.float64)
        if a.shape != (16,):
            raise ValueError(f"symmetries_discrete[{k}] must hold 16 numbers, got shape {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"symmetries_discrete[{k}] holds a non-finite number")
        disc.append(a.reshape(4, 4))
    cont = []
    steps = int(math.ceil(math.pi / max_sym_disc_step))
    for k, sym in enumerate(model_info.get("symmetries_continuous", []) or []):
        if not isinstance(sym, dict) or "axis" not in sym or "offset" not in sym:
            raise ValueError(f"symmetries_continuous[{k}] must be {{'axis', 'offset'}}")
        axis, off = np.asarray(sym["axis"], dtype=np.float64), np.asarray(sym["offset"], dtype=np.float64)
        if axis.shape != (3,) or off.shape != (3,):
            raise ValueError(f"symmetries_continuous[{k}]: axis and offset must hold 3 numbers each")
        if not (np.all(np.isfinite(axis)) and np.all(np.isfinite(off))):
            raise ValueError(f"symmetries_continuous[{k}] holds a non-finite number")
        n = float(np.linalg.norm(axis))
        if n == 0.0:
            raise ValueError(f"symmetries_continuous[{k}]: the axis is zero")
        axis = axis / n
        for i in range(steps):
            T = np.eye(4)
            T[:3, :3] = _rotation(axis, i * 2.0 * math.pi / steps)
            T[:3, 3] = off - T[:3, :3] @ off
            cont.append(T)
    if not cont:
        return np.stack(disc)
    return np.stack([c @ d for d in disc for c in cont])


class ObjectModels:
    """The models of a dataset, uploaded once: {obj_id: {"vertices": (Nv, 3) millimetres (as template_bank.load_ply returns them),
    "info": the object's models_info.json entry, optionally "faces": (Nf, 3) integer vertex indices (as load_ply returns them; needed
    by vsd_errors and render_depth only — `has_faces` says whether every object has them)}}.  Holds every object's vertices (and
    faces, indices local to their object) concatenated, their symmetry transforms
    (symmetry_transforms) concatenated as float32 (R, t), the offset tables and the diameters (`info["diameter"]`).
    max_points: None, or a bound on the vertices ADD-S runs on: every ceil(Nv / max_points)-th vertex is kept (deterministic);
    the other errors always use every vertex, and pose_errors reports the bound under "adds_max_points"."""

    def __init__(self, objects, max_sym_disc_step=0.01, max_points=None, device="cuda"):
        if not isinstance(objects, dict) or not objects:
            raise ValueError("objects must be a non-empty {obj_id: {'vertices', 'info'}} dict")
        if max_points is not None and (not isinstance(max_points, int) or max_points <= 0):
            raise ValueError(f"max_points must be None or a positive int, got {max_points!r}")
        self.obj_ids = [int(k) for k in objects]
        self.index = {o: k for k, o in enumerate(self.obj_ids)}
        self.max_points, self.device = max_points, torch.device(device)
        verts, sub, syms, diam, faces = [], [], [], [], []
        for key, obj in objects.items():
            v = np.asarray(obj["vertices"])
            if v.ndim != 2 or v.shape[1] != 3 or len(v) == 0 or not np.issubdtype(v.dtype, np.floating):
                raise ValueError(f"object {key}: vertices must be a non-empty (Nv, 3) float array, got {v.dtype} {v.shape}")
            if not np.all(np.isfinite(v)):
                raise ValueError(f"object {key}: vertices contain a non-finite value")
            info = obj.get("info") or {}
            d = float(info.get("diameter", float("nan")))
            if not (math.isfinite(d) and d > 0):
                raise ValueError(f"object {key}: info['diameter'] must be a positive number")
            v = np.ascontiguousarray(v, dtype=np.float32)
            verts.append(v)
            f = obj.get("faces")
            if f is None:
                f = np.zeros((0, 3), dtype=np.int32)
            else:
                f = np.asarray(f)
                if f.ndim != 2 or f.shape[1] != 3 or len(f) == 0 or not np.issubdtype(f.dtype, np.integer):
                    raise ValueError(f"object {key}: faces must be a non-empty (Nf, 3) integer array, got {f.dtype} {f.shape}")
                if f.min() < 0 or f.max() >= len(v):
                    raise ValueError(f"object {key}: a face index lies outside [0, {len(v)})")
                f = np.ascontiguousarray(f, dtype=np.int32)
            faces.append(f)
            sub.append(v if max_points is None else np.ascontiguousarray(v[::-(-len(v) // max_points)]))
            syms.append(symmetry_transforms(info, max_sym_disc_step))
            diam.append(d)
        self.symmetries = syms                                   # per object (S, 4, 4) float64
        self.diameters = np.array(diam, dtype=np.float64)
        self.vert_off = self._offsets(verts)
        self.adds_off = self.vert_off if max_points is None else self._offsets(sub)
        self.sym_off = self._offsets(syms)
        self.face_off = self._offsets(faces)
        self.faces_host = np.concatenate(faces)
        self.face_counts = (self.face_off[1:] - self.face_off[:-1]).astype(np.int64)
        self.has_faces = all(len(f) for f in faces)
        self.diameters_f32 = self.diameters.astype(np.float32)
        self.aabb_corners = [np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], dtype=np.float64)
                             for lo, hi in ((v.min(axis=0), v.max(axis=0)) for v in verts)]          # per object (8, 3)
        sym = np.concatenate(syms)
        self.sym_R_host = np.ascontiguousarray(sym[:, :3, :3].reshape(-1, 9).astype(np.float32))
        self.sym_t_host = np.ascontiguousarray(sym[:, :3, 3].astype(np.float32))
        self.vertices_host = np.concatenate(verts)
        self.adds_vertices_host = self.vertices_host if max_points is None else np.concatenate(sub)
        up = lambda a: torch.from_numpy(a).to(self.device)      # noqa: E731
        self.vertices = up(self.vertices_host)
        self.adds_vertices = self.vertices if max_points is None else up(self.adds_vertices_host)
        self.sym_R, self.sym_t = up(self.sym_R_host), up(self.sym_t_host)
        self.vert_off_d, self.sym_off_d = up(self.vert_off), up(self.sym_off)
        self.adds_off_d = self.vert_off_d if max_points is None else up(self.adds_off)
        self.faces = up(self.faces_host) if len(self.faces_host) else None
        self.face_off_d, self.diameters_d = up(self.face_off), up(self.diameters_f32)

    @staticmethod
    def _offsets(parts):
        off = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        if off[-1] >= 2 ** 31:
            raise ValueError("the concatenated models exceed 2^31 rows")
        return off.astype(np.int32)

    def n_symmetries(self, obj_id):
        k = self.index[int(obj_id)]
        return int(self.sym_off[k + 1] - self.sym_off[k])

    def diameter(self, obj_id):
        return float(self.diameters[self.index[int(obj_id)]])

    def n_faces(self, obj_id):
        k = self.index[int(obj_id)]
        return int(self.face_off[k + 1] - self.face_off[k])


def _plan_chunks(models, pair_obj, mask, workspace_bytes):
    """-> (pairs per launch sequence, bytes of the workspace for that many) under the bound `workspace_bytes` (at least one pair)."""
    ns = (models.sym_off[1:] - models.sym_off[:-1])[pair_obj]
    na = (models.adds_off[1:] - models.adds_off[:-1])[pair_obj]
    S_max, A_max = int(ns.max()), int(na.max())
    one = _lib.workspace_bytes("pp_pose_errors_workspace_bytes", 1, S_max, A_max, mask)
    chunk = max(1, min(len(pair_obj), int(workspace_bytes) // one, (2 ** 31 - 1) // S_max))
    return chunk, _lib.workspace_bytes("pp_pose_errors_workspace_bytes", chunk, S_max, A_max, mask)


def pose_error_chunks(models, obj_ids, kinds=("mssd", "mspd"), workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """How many launch sequences pose_errors makes for these pairs under `workspace_bytes` (1: everything in one)."""
    kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
    pair_obj = np.array([models.index[int(o)] for o in np.asarray(obj_ids).tolist()], dtype=np.int32)
    if len(pair_obj) == 0:
        return 0
    chunk, _ = _plan_chunks(models, pair_obj, sum(KINDS[k] for k in set(kinds)), workspace_bytes)
    return -(-len(pair_obj) // chunk)


def pose_errors(models, obj_ids, R_est, t_est, R_gt, t_gt, K=None, kinds=("mssd", "mspd"), workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """The errors of P (estimate, ground truth) pairs, whatever objects they mix, in one launch sequence (one compose launch, one
    launch per kind, one finalize launch) -> {kind: (P,) float32 device tensor}, plus "mssd_sym" / "mspd_sym" (P,) int32: the index
    of the minimising symmetry within symmetry_transforms' list (the lowest on a tie), plus "adds_max_points" when ADD-S is asked.

    obj_ids: P ids known to `models`.  R_* (P, 3, 3), t_* (P, 3) float arrays or tensors, millimetres.  K: (3, 3) or (P, 3, 3),
    required for "mspd"; arrays and tensors must be float, nested lists are read as float64; only fx = K[0, 0] and fy = K[1, 1] enter (no skew; the principal point cancels in the difference).
    kinds: any of "mssd", "mspd", "add", "adds".  A symmetry under which a point of either pose has z <= 0 has MSPD +inf; a pair
    has +inf when all have.  A pose that holds a NaN or an infinity gives MSSD +inf (MSPD +inf, ADD / ADD-S NaN or +inf): it can never
    fall below a threshold, and match_and_score never matches it.  The composed-transform workspace is 56 bytes per (pair, symmetry):
    when P needs more than `workspace_bytes` the pairs are processed in chunks (pose_error_chunks says how many), with identical results.  P = 0: empty tensors, no launch.
    ValueError: a shape or dtype mismatch, an unknown obj_id or kind ("vsd" among them: it needs images, see vsd_errors), "mspd" without K."""
    if not isinstance(models, ObjectModels):
        raise ValueError("models must be an ObjectModels")
    kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
    for k in kinds:
        if k not in KINDS:
            raise ValueError(f"unknown kind {k!r}: choose from {sorted(KINDS)}")
    if not kinds:
        raise ValueError("no kind requested")
    if isinstance(obj_ids, torch.Tensor):
        obj_ids = obj_ids.cpu().numpy()
    ids = np.asarray(obj_ids)
    if ids.ndim != 1 or (len(ids) and not np.issubdtype(ids.dtype, np.integer)):
        raise ValueError(f"obj_ids must be a 1-D integer sequence, got {ids.dtype} {ids.shape}")
    P, dev = len(ids), models.device
    for o in ids:
        if int(o) not in models.index:
            raise ValueError(f"unknown obj_id {int(o)}: the models hold {models.obj_ids}")
    pair_obj = np.array([models.index[int(o)] for o in ids], dtype=np.int32)
    Re, te = scn.pose_tensor("R_est", R_est, P, (3, 3), dev), scn.pose_tensor("t_est", t_est, P, (3,), dev)
    Rg, tg = scn.pose_tensor("R_gt", R_gt, P, (3, 3), dev), scn.pose_tensor("t_gt", t_gt, P, (3,), dev)
    focal = None
    if "mspd" in kinds:
        if K is None:
            raise ValueError("kind 'mspd' needs the camera matrix K")
        Kt = scn.pose_tensor("K", K, P, [(3, 3), (P, 3, 3)], dev)
        if Kt.dim() == 2:
            Kt = Kt[None].expand(P, 3, 3)
        focal = torch.stack([Kt[:, 0, 0], Kt[:, 1, 1]], dim=1).contiguous()
    out = {}
    for k in kinds:
        out[k] = torch.empty(P, dtype=torch.float32, device=dev)
        if k in ("mssd", "mspd"):
            out[k + "_sym"] = torch.empty(P, dtype=torch.int32, device=dev)
    if "adds" in kinds:
        out["adds_max_points"] = models.max_points
    if P == 0:
        return out
    scn.require_gpu(dev)
    mask = sum(KINDS[k] for k in set(kinds))
    chunk, need = _plan_chunks(models, pair_obj, mask, workspace_bytes)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    pair_obj_d = torch.from_numpy(pair_obj).to(dev)

    for p0 in range(0, P, chunk):
        n = min(chunk, P - p0)
        at = lambda t: None if t is None else t[p0:]             # noqa: E731  (an optional per-pair table from pair p0 on)
        _lib.call("pp_pose_errors", models.vertices, models.vert_off_d, models.adds_vertices, models.adds_off_d, models.sym_R, models.sym_t,
                  models.sym_off_d, models.vert_off, models.adds_off, models.sym_off, len(models.obj_ids), pair_obj_d[p0:], pair_obj[p0:],
                  Re[p0:], te[p0:], Rg[p0:], tg[p0:], at(focal), n, mask, ws, ws.numel(), at(out.get("mssd")), at(out.get("mssd_sym")),
                  at(out.get("mspd")), at(out.get("mspd_sym")), at(out.get("add")), at(out.get("adds")))
    return out


# ---- VSD: depth renders and visibility ---------------------------------------------------------------------------------------------
def _vsd_launch(models, cams, H, W, view_obj, view_img, poses, windows, groups, near, pair_est=None, pair_gt=None, depth=None,
                delta=15.0, taus=None, want_depth=False):
    """One pp_vsd_errors call per group -> (vsd, counts, per-view near counts, dense depth or None), device tensors."""
    dev = models.device
    scn.require_gpu(dev)
    U, P = len(view_obj), 0 if pair_est is None else len(pair_est)
    T = 1 if taus is None else len(taus)
    taus_h = np.ascontiguousarray(np.zeros(1) if taus is None else taus, dtype=np.float32)
    vsd = torch.empty((P, T), dtype=torch.float32, device=dev)
    counts = torch.empty((P, 2 + T), dtype=torch.int32, device=dev)
    near_all = torch.zeros(U, dtype=torch.int32, device=dev)
    dense = torch.empty((U, H, W), dtype=torch.float32, device=dev) if want_depth else None
    for views, pairs in groups:
        packed = scn.PackedScene(models, cams, H, W, near, view_obj[views], view_img[views], poses[views], windows[views])
        ws = torch.empty(_lib.workspace_bytes("pp_vsd_workspace_bytes", packed.samples, packed.faces), dtype=torch.uint8, device=dev)
        near_d = torch.empty(len(views), dtype=torch.int32, device=dev)
        pe = pg = pe_d = pg_d = vsd_at = counts_at = dense_at = None
        n_pairs = 0
        if pairs is not None:
            local = {int(v): k for k, v in enumerate(views.tolist())}
            pe = np.array([local[int(v)] for v in pair_est[pairs]], dtype=np.int32)
            pg = np.array([local[int(v)] for v in pair_gt[pairs]], dtype=np.int32)
            pe_d, pg_d, n_pairs, p0 = torch.from_numpy(pe).to(dev), torch.from_numpy(pg).to(dev), len(pairs), int(pairs[0])
            vsd_at, counts_at = vsd[p0:], counts[p0:]
        if want_depth:                                            # (render_depth: the groups are consecutive views)
            dense_at = dense[int(views[0]):]
        _lib.call("pp_vsd_errors", packed.scene, pe_d, pg_d, pe, pg, n_pairs, depth, float(delta), taus_h, T, ws, ws.numel(),
                  vsd_at, counts_at, near_d, dense_at)
        near_all[torch.from_numpy(views).to(dev)] = near_d
    return vsd, counts, near_all, dense


def render_depth(models, obj_ids, R, t, K, resolution, image_index=None, near=1.0, window="auto",
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """Depth renders of U (object, pose) views -> {"depth": (U, H, W) float32 device tensor, camera Z in millimetres, 0 = background,
    "near_count": the triangles dropped because a vertex had Zc <= near}.  resolution = (H, W); K (3, 3) or (n_images, 3, 3) with
    image_index (U,) choosing the camera of each view (default: image 0); R (U, 3, 3), t (U, 3) millimetres; near in millimetres.
    window: "auto" samples the host-planned window of each view (plan_window), "full" the whole frame — the same bits.  The views are
    rendered in as many launch sequences as `workspace_bytes` needs.  U = 0: an empty tensor, no launch.  ValueError as vsd_errors."""
    obj = scn.obj_index(models, obj_ids)
    U = len(obj)
    scn.check_scalars(near, window, workspace_bytes)
    res = scn.resolution_hw(resolution)
    if res is None:
        raise ValueError(f"resolution must be (H, W), got {resolution!r}")
    H, W = res
    if not scn.frame_in_range(H, W):
        raise ValueError(f"resolution must be positive with H W < 2^31, got {(H, W)}")
    Rh, th = scn.host_f32("R", R, U, (3, 3)), scn.host_f32("t", t, U, (3,))
    n_images = scn.n_images_of(K)
    cams = scn.cameras(K, n_images)
    img = scn.image_index(image_index, U, n_images)
    if U == 0:
        return {"depth": torch.empty((0, H, W), dtype=torch.float32, device=models.device), "near_count": 0}
    poses = scn.pose44(Rh, th)
    windows = scn.view_windows(models, obj, img, poses, cams, H, W, near, window)
    groups = scn.view_groups(models, obj, windows, None, None, workspace_bytes)
    _, _, near_all, dense = _vsd_launch(models, cams, H, W, obj, img, poses, windows, groups, near, want_depth=True)
    return {"depth": dense, "near_count": int(near_all.sum().item())}


def vsd_errors(models, obj_ids, R_est, t_est, R_gt, t_gt, K, depth, image_index=None, depth_scale=None, delta=15.0, taus=VSD_TAUS,
               near=1.0, window="auto", workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """The BOP19 VSD of P (estimate, ground truth) pairs over n_images test depth images -> {"vsd": (P, T) float32 e_tau,
    "visib_union", "visib_inter": (P,) int32, "n_far": (P, T) int32 (intersection pixels with |D_gt - D_est| / diameter >= tau)
    device tensors, "n_views": the distinct views rendered, "near_count": the triangles dropped at the near plane over those views,
    "n_groups": the pp_vsd_errors calls made (1 unless the views exceed `workspace_bytes`)}.

    depth: (n_images, H, W), uint16 raw values with `depth_scale` (millimetres per unit, a number or one per image) or float millimetres
    (depth_scale None); numpy or tensor; a value that is not > 0 is missing.  K: (3, 3) or (n_images, 3, 3); image_index (P,): the image
    of each pair (default 0).  delta (mm) and taus (T <= 16, fractions of the diameter) as in the definition (include/picopose_hip.h).
    Identical (image, object, pose bytes) views are rendered once: a ground truth shared by several estimates, an estimate paired with
    several instances.  window "auto": each view is sampled inside its host-planned window (plan_window); "full": the whole frame — the
    same bits.  A pose holding a NaN or an infinity gets an empty window: it renders nothing and e = 1 for every tau.  When the views of
    all pairs need more than `workspace_bytes` the pairs are processed in groups, with identical results.  P = 0: empty tensors, no launch.
    ValueError: an object without faces, an unknown obj_id, shape or dtype mismatches, image_index out of range, T outside 1..16."""
    obj = scn.obj_index(models, obj_ids)
    P, dev = len(obj), models.device
    scn.check_scalars(near, window, workspace_bytes)
    if not (isinstance(delta, (int, float)) and math.isfinite(delta) and delta > 0):
        raise ValueError(f"delta must be a positive number, got {delta!r}")
    tau = np.asarray(taus, dtype=np.float64)
    if tau.ndim != 1 or not 1 <= len(tau) <= VSD_MAX_TAUS or not np.all(np.isfinite(tau)):
        raise ValueError(f"taus must be 1 .. {VSD_MAX_TAUS} finite numbers, got shape {tau.shape}")
    T = len(tau)
    Re, te = scn.host_f32("R_est", R_est, P, (3, 3)), scn.host_f32("t_est", t_est, P, (3,))
    Rg, tg = scn.host_f32("R_gt", R_gt, P, (3, 3)), scn.host_f32("t_gt", t_gt, P, (3,))
    n_images, H, W, scale = scn.check_depth(depth, depth_scale)
    cams = scn.cameras(K, n_images)
    img = scn.image_index(image_index, P, n_images)
    if P == 0:
        z = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)     # noqa: E731
        return {"vsd": torch.empty((0, T), dtype=torch.float32, device=dev), "visib_union": z(0), "visib_inter": z(0), "n_far": z(0, T),
                "n_views": 0, "near_count": 0}
    scn.require_gpu(dev)
    depth_d = scn.depth_mm(depth, scale, dev)
    # the distinct views: (image, object, bytes of the float32 pose)
    Pe, Pg = scn.pose44(Re, te), scn.pose44(Rg, tg)
    index, view_obj, view_img, poses = {}, [], [], []
    pair_est, pair_gt = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
    for p in range(P):
        for dst, pose in ((pair_est, Pe[p]), (pair_gt, Pg[p])):
            key = (int(img[p]), int(obj[p]), pose.tobytes())
            v = index.get(key)
            if v is None:
                v = index[key] = len(poses)
                view_obj.append(obj[p])
                view_img.append(img[p])
                poses.append(pose)
            dst[p] = v
    view_obj, view_img, poses = np.array(view_obj, dtype=np.int32), np.array(view_img, dtype=np.int32), np.stack(poses)
    windows = scn.view_windows(models, view_obj, view_img, poses, cams, H, W, near, window)
    groups = scn.view_groups(models, view_obj, windows, pair_est, pair_gt, workspace_bytes)
    vsd, counts, near_all, _ = _vsd_launch(models, cams, H, W, view_obj, view_img, poses, windows, groups, near, pair_est, pair_gt,
                                           depth_d, delta, tau, want_depth=False)
    return {"vsd": vsd, "visib_union": counts[:, 0], "visib_inter": counts[:, 1], "n_far": counts[:, 2:], "n_views": len(poses),
            "near_count": int(near_all.sum().item()), "n_groups": len(groups)}


# ---- parsers: JSON and CSV only ----------------------------------------------------------------------------------------------------
def read_bop_results(path_or_lines):
    """BOP results rows `scene_id,im_id,obj_id,score,R (9 numbers),t (3 numbers, mm),time` (what pipeline.bop_csv_lines writes; a
    header line is skipped) from a file path or an iterable of lines -> {"scene_id", "im_id", "obj_id" (N,) int64, "score", "time"
    (N,) float64, "R" (N, 3, 3), "t" (N, 3) float64}."""
    if isinstance(path_or_lines, (str, os.PathLike)):
        with open(path_or_lines) as fh:
            lines = fh.readlines()
    else:
        lines = list(path_or_lines)
    rows = []
    for n, line in enumerate(lines):
        line = line.strip()
        if not line or line.startswith("scene_id"):
            continue
        f = line.split(",")
        if len(f) != 7:
            raise ValueError(f"results line {n + 1}: expected 7 comma-separated fields, got {len(f)}")
        R, t = f[4].split(), f[5].split()
        if len(R) != 9 or len(t) != 3:
            raise ValueError(f"results line {n + 1}: R must hold 9 numbers and t 3")
        rows.append((int(f[0]), int(f[1]), int(f[2]), float(f[3]), [float(v) for v in R], [float(v) for v in t], float(f[6])))
    return {"scene_id": np.array([r[0] for r in rows], dtype=np.int64), "im_id": np.array([r[1] for r in rows], dtype=np.int64),
            "obj_id": np.array([r[2] for r in rows], dtype=np.int64), "score": np.array([r[3] for r in rows], dtype=np.float64),
            "R": np.array([r[4] for r in rows], dtype=np.float64).reshape(-1, 3, 3),
            "t": np.array([r[5] for r in rows], dtype=np.float64).reshape(-1, 3), "time": np.array([r[6] for r in rows], dtype=np.float64)}


def _json(path_or_obj):
    if isinstance(path_or_obj, (str, os.PathLike)):
        with open(path_or_obj) as fh:
            return json.load(fh)
    return path_or_obj


def read_scene_gt(path):
    """scene_gt.json -> {im_id: {"obj_id" (n,) int64, "R" (n, 3, 3), "t" (n, 3) float64 millimetres}}, instances in file order."""
    out = {}
    for im, insts in _json(path).items():
        out[int(im)] = {"obj_id": np.array([int(g["obj_id"]) for g in insts], dtype=np.int64),
                        "R": np.array([g["cam_R_m2c"] for g in insts], dtype=np.float64).reshape(-1, 3, 3),
                        "t": np.array([g["cam_t_m2c"] for g in insts], dtype=np.float64).reshape(-1, 3)}
    return out


def read_scene_camera(path):
    """scene_camera.json -> {im_id: {"K" (3, 3) float64, "depth_scale" float}}."""
    return {int(im): {"K": np.array(c["cam_K"], dtype=np.float64).reshape(3, 3), "depth_scale": float(c.get("depth_scale", 1.0))}
            for im, c in _json(path).items()}


def read_targets(path):
    """test_targets_bop19.json -> (N, 4) int64 rows {scene_id, im_id, obj_id, inst_count}, in file order."""
    return np.array([[int(t["scene_id"]), int(t["im_id"]), int(t["obj_id"]), int(t["inst_count"])] for t in _json(path)],
                    dtype=np.int64).reshape(-1, 4)


# ---- the BOP localization protocol -------------------------------------------------------------------------------------------------
def plan_pairs(estimates, ground_truth, targets):
    """Host side of match_and_score: per target {scene_id, im_id, obj_id, inst_count} the inst_count estimates of that object in that
    image with the highest score (ties: file order), each paired with every ground-truth instance of the object in the image ->
    {"target", "est", "gt" (n_pairs,) int64: target row, estimate row, instance index within the image's scene_gt entry}."""
    tg, es, gs = [], [], []
    key = {}
    for i, k in enumerate(zip(estimates["scene_id"].tolist(), estimates["im_id"].tolist(), estimates["obj_id"].tolist())):
        key.setdefault(k, []).append(i)
    for n, (scene, im, obj, count) in enumerate(np.asarray(targets, dtype=np.int64).reshape(-1, 4).tolist()):
        rows = key.get((scene, im, obj), [])
        rows = sorted(rows, key=lambda i: (-estimates["score"][i], i))[:count]
        gt = ground_truth.get(scene, {}).get(im)
        inst = [] if gt is None else np.where(gt["obj_id"] == obj)[0].tolist()
        for e in rows:
            for g in inst:
                tg.append(n)
                es.append(e)
                gs.append(g)
    return {"target": np.array(tg, dtype=np.int64), "est": np.array(es, dtype=np.int64), "gt": np.array(gs, dtype=np.int64)}


def score_pairs(pairs, errors, limits, scores, targets):
    """Greedy matching per threshold.  pairs: plan_pairs' result; errors (n_pairs,); limits (n_pairs, T): the error a pair must stay
    BELOW at each threshold; scores: every estimate's score.  Per target the kept estimates are visited in order of descending score
    (ties: file order); each takes the unused ground-truth instance with the lowest error (ties: the lowest index) when that error
    is below the limit.  -> (n_targets, T) int64 matched counts."""
    targets = np.asarray(targets).reshape(-1, 4)
    T = limits.shape[1] if len(limits) else 0
    matched = np.zeros((len(targets), T), dtype=np.int64)
    order = np.lexsort((pairs["gt"], pairs["est"], pairs["target"]))
    by_target = {}
    for i in order.tolist():
        by_target.setdefault(int(pairs["target"][i]), {}).setdefault(int(pairs["est"][i]), []).append(i)
    for n, per_est in by_target.items():
        ests = sorted(per_est, key=lambda e: (-scores[e], e))
        for k in range(T):
            used = set()
            for e in ests:
                best = None
                for i in per_est[e]:
                    g = int(pairs["gt"][i])
                    if g in used or not errors[i] < limits[i, k]:
                        continue
                    if best is None or errors[i] < errors[best]:
                        best = i
                if best is not None:
                    used.add(int(pairs["gt"][best]))
                    matched[n, k] += 1
    return matched


def match_and_score(estimates, ground_truth, targets, models, cameras, image_width=640, workspace_bytes=DEFAULT_WORKSPACE_BYTES,
                    depth_images=None, vsd_delta=15.0, vsd_taus=VSD_TAUS, images_per_call=64):
    """The BOP localization protocol for MSSD and MSPD.  estimates: read_bop_results' dict; ground_truth / cameras:
    {scene_id: read_scene_gt(...) / read_scene_camera(...)}; targets: read_targets' rows; models: ObjectModels.

    Per target the inst_count best-scored estimates are kept and paired with every ground-truth instance of that object in that image;
    the errors of ALL pairs of all images come from one pose_errors call; an estimate is correct at a threshold when its error is below
    it (MSSD: 0.05 .. 0.5 of the object's diameter in steps of 0.05; MSPD: 5 r .. 50 r px in steps of 5 r, r = image_width / 640), matched
    greedily (score_pairs).  Recall = matched / sum of inst_count.  -> {"AR_MSSD", "AR_MSPD": mean recall over the thresholds,
    "recall_mssd", "recall_mspd" (10,), "thresholds_mssd", "thresholds_mspd", "per_object": {obj_id: the same four and "targets"},
    "pairs": plan_pairs' arrays plus "mssd", "mspd" (float32 numpy), "n_targets": sum of inst_count, "vsd": None}.
    Without depth_images VSD is not computed ("vsd" is None) and there is no three-term average: AR_MSSD and AR_MSPD are two of its terms.

    depth_images: {scene_id: {im_id: (H, W) array}} or a callable (scene_id, im_id) -> (H, W) array: the test depth images, uint16 raw
    or float raw values, scaled by cameras[scene][im]["depth_scale"] to millimetres (decoding the PNGs stays with the caller).  Only the
    images that occur in pairs are asked for, images_per_call at a time, one vsd_errors call each (delta = vsd_delta, taus = vsd_taus;
    the models need faces).  A pair is correct at (tau, theta) when e_tau < theta, theta = VSD_THRESHOLDS; matching is score_pairs per tau.
    Adds "vsd": {"errors" (n_pairs, T), "taus", "thresholds", "delta"}, "recall_vsd" (T, 10), "AR_VSD", "AR" = (AR_VSD + AR_MSSD +
    AR_MSPD) / 3, and the last three per object."""
    targets = np.asarray(targets, dtype=np.int64).reshape(-1, 4)
    pairs = plan_pairs(estimates, ground_truth, targets)
    n = len(pairs["est"])
    obj = targets[pairs["target"], 2] if n else np.zeros(0, dtype=np.int64)
    R_gt, t_gt, K = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 3, 3))
    for i in range(n):
        scene, im = int(targets[pairs["target"][i], 0]), int(targets[pairs["target"][i], 1])
        gt = ground_truth[scene][im]
        R_gt[i], t_gt[i] = gt["R"][pairs["gt"][i]], gt["t"][pairs["gt"][i]]
        if scene not in cameras or im not in cameras[scene]:
            raise ValueError(f"cameras holds no entry for scene {scene}, image {im}, which has estimates to score")
        K[i] = cameras[scene][im]["K"]
    err = pose_errors(models, obj, estimates["R"][pairs["est"]], estimates["t"][pairs["est"]], R_gt, t_gt, K=K, kinds=("mssd", "mspd"),
                      workspace_bytes=workspace_bytes)
    mssd, mspd = err["mssd"].cpu().numpy(), err["mspd"].cpu().numpy()
    vsd = None
    if depth_images is not None:
        if not (isinstance(images_per_call, int) and images_per_call > 0):
            raise ValueError(f"images_per_call must be a positive int, got {images_per_call!r}")
        taus = np.asarray(vsd_taus, dtype=np.float64)
        if taus.ndim != 1 or not 1 <= len(taus) <= VSD_MAX_TAUS:
            raise ValueError(f"vsd_taus must hold 1 .. {VSD_MAX_TAUS} numbers, got shape {taus.shape}")
        where = [(int(targets[pairs["target"][i], 0]), int(targets[pairs["target"][i], 1])) for i in range(n)]
        images = list(dict.fromkeys(where))                       # the images that occur in pairs, in order of first use
        e = np.ones((n, len(taus)), dtype=np.float32)
        for b0 in range(0, len(images), images_per_call):
            batch = images[b0:b0 + images_per_call]
            slot = {k: j for j, k in enumerate(batch)}
            rows = np.array([i for i in range(n) if where[i] in slot], dtype=np.int64)
            frames = [np.asarray(depth_images(*k) if callable(depth_images) else depth_images[k[0]][k[1]]) for k in batch]
            if any(f.ndim != 2 or f.shape != frames[0].shape for f in frames):
                raise ValueError("depth images of one call must share one (H, W) resolution")
            scale = np.array([cameras[k[0]][k[1]]["depth_scale"] for k in batch], dtype=np.float64)
            if all(f.dtype == np.uint16 for f in frames):
                depth, depth_scale = np.stack(frames), scale
            else:
                depth = np.stack([f.astype(np.float32) * np.float32(sc) for f, sc in zip(frames, scale)])
                depth_scale = None
            Kb = np.stack([cameras[k[0]][k[1]]["K"] for k in batch]).astype(np.float64)
            r = vsd_errors(models, obj[rows], estimates["R"][pairs["est"][rows]], estimates["t"][pairs["est"][rows]], R_gt[rows], t_gt[rows],
                           Kb, depth, image_index=np.array([slot[where[i]] for i in rows], dtype=np.int32), depth_scale=depth_scale,
                           delta=vsd_delta, taus=taus, workspace_bytes=workspace_bytes)
            e[rows] = r["vsd"].cpu().numpy()
        vsd = {"errors": e, "taus": taus.copy(), "thresholds": VSD_THRESHOLDS.copy(), "delta": float(vsd_delta)}
    return score_errors(pairs, mssd, mspd, estimates["score"], targets, models, image_width, vsd=vsd)


def score_errors(pairs, mssd, mspd, scores, targets, models, image_width=640, vsd=None):
    """match_and_score's host half: the recalls from the per-pair errors (numpy arrays).  vsd: None, or {"errors" (n_pairs, T), "taus",
    "thresholds" (10,), "delta"}: per tau the pairs are matched by score_pairs with the thresholds as limits."""
    targets = np.asarray(targets, dtype=np.int64).reshape(-1, 4)
    n = len(pairs["est"])
    obj = targets[pairs["target"], 2] if n else np.zeros(0, dtype=np.int64)
    diam = np.array([models.diameter(o) for o in obj], dtype=np.float64)
    r = float(image_width) / 640.0
    lim_mssd = diam[:, None] * MSSD_THRESHOLDS[None]
    lim_mspd = np.broadcast_to(MSPD_THRESHOLDS[None] * r, (n, 10))
    hit = {"mssd": score_pairs(pairs, np.asarray(mssd, dtype=np.float64), lim_mssd, scores, targets),
           "mspd": score_pairs(pairs, np.asarray(mspd, dtype=np.float64), lim_mspd, scores, targets)}
    total = int(targets[:, 3].sum())
    hit_vsd = None
    if vsd is not None:
        ev, th = np.asarray(vsd["errors"], dtype=np.float64).reshape(n, -1), np.asarray(vsd["thresholds"], dtype=np.float64)
        lim = np.broadcast_to(th[None], (n, len(th)))
        hit_vsd = np.stack([score_pairs(pairs, ev[:, k], lim, scores, targets) for k in range(ev.shape[1])], axis=1)   # (targets, T, 10)

    def recalls(rows):
        cnt = int(targets[rows, 3].sum())
        rec = {k: (hit[k][rows].sum(axis=0) / cnt if cnt else np.zeros(10)) for k in hit}
        out = {"AR_MSSD": float(rec["mssd"].mean()), "AR_MSPD": float(rec["mspd"].mean()), "recall_mssd": rec["mssd"],
               "recall_mspd": rec["mspd"], "targets": cnt}
        if hit_vsd is not None:
            out["recall_vsd"] = hit_vsd[rows].sum(axis=0) / cnt if cnt else np.zeros(hit_vsd.shape[1:])
            out["AR_VSD"] = float(out["recall_vsd"].mean())
            out["AR"] = (out["AR_VSD"] + out["AR_MSSD"] + out["AR_MSPD"]) / 3.0
        return out

    res = recalls(np.arange(len(targets)))
    res["n_targets"] = total
    del res["targets"]
    res["thresholds_mssd"], res["thresholds_mspd"] = MSSD_THRESHOLDS.copy(), MSPD_THRESHOLDS * r
    res["per_object"] = {int(o): recalls(np.where(targets[:, 2] == o)[0]) for o in np.unique(targets[:, 2])}
    res["pairs"] = dict(pairs, mssd=np.asarray(mssd), mspd=np.asarray(mspd))
    res["vsd"] = None if vsd is None else dict(vsd)
    return res
