"""Oracle of picopose_amd/evaluation.py (a helper, not collected).

Part 1 restates the definitions in numpy float64: the symmetry set of a models_info entry, MSSD, MSPD, ADD, ADD-S and the BOP
localization matching.  Part 2 restates the KERNEL's arithmetic (include/picopose_hip.h, "THE ARITHMETIC") in numpy float32, one
ufunc per operation so that nothing is contracted: MSSD, MSPD and their symmetry indices must equal it bit for bit.  Part 3 holds the
float32 error bounds the GPU tests assert.

Nearest neighbours (ADD-S) are brute force up to BRUTE vertices and an exact k-d tree search (scipy.spatial.cKDTree) above."""
import math

import numpy as np

F = np.float32
EPS = 2.0 ** -24
BRUTE = 2048


# ---- part 1: the definitions, float64 ---------------------------------------------------------------------------------------------
def axis_rotation(axis, angle):
    """Rotation by `angle` about the unit vector `axis`, column by column from v cos + (a x v) sin + a (a . v)(1 - cos)."""
    a = np.asarray(axis, dtype=np.float64)
    cols = [v * math.cos(angle) + np.cross(a, v) * math.sin(angle) + a * np.dot(a, v) * (1.0 - math.cos(angle)) for v in np.eye(3)]
    return np.stack(cols, axis=1)


def symmetry_set(info, step=0.01):
    """Identity + symmetries_discrete; with symmetries_continuous every product continuous x discrete (discrete-major), the continuous
    ones being ceil(pi / step) equal rotation steps about the axis through the offset."""
    disc = [np.eye(4)] + [np.asarray(s, dtype=np.float64).reshape(4, 4) for s in info.get("symmetries_discrete", [])]
    cont = []
    n = int(math.ceil(math.pi / step))
    for c in info.get("symmetries_continuous", []):
        a = np.asarray(c["axis"], dtype=np.float64)
        a, off = a / np.linalg.norm(a), np.asarray(c["offset"], dtype=np.float64)
        for k in range(n):
            T = np.eye(4)
            T[:3, :3] = axis_rotation(a, 2.0 * math.pi * k / n)
            T[:3, 3] = off - T[:3, :3] @ off                   # x -> R (x - off) + off
            cont.append(T)
    return np.stack(disc) if not cont else np.stack([c @ d for d in disc for c in cont])


def _nn_dist(a, b):
    """Per row of a the distance to the nearest row of b (float64)."""
    if len(b) <= BRUTE:
        return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1).min(axis=1))
    from scipy.spatial import cKDTree

    return cKDTree(b).query(a, k=1)[0]


def errors64(V, syms, Re, te, Rg, tg, K=None, kinds=("mssd", "mspd", "add", "adds"), V_adds=None):
    """One pair, straight from the definitions.  V (Nv, 3), syms (S, 4, 4), K (3, 3) -> dict of floats (+ *_sym indices)."""
    V, syms = np.asarray(V, dtype=np.float64), np.asarray(syms, dtype=np.float64)
    Re, te, Rg, tg = (np.asarray(a, dtype=np.float64) for a in (Re, te, Rg, tg))
    out = {}
    e = V @ Re.T + te
    if "mssd" in kinds or "mspd" in kinds:
        sv = np.einsum("sij,nj->sni", syms[:, :3, :3], V) + syms[:, None, :3, 3]          # S x
        g = sv @ Rg.T + tg
    if "mssd" in kinds:
        with np.errstate(invalid="ignore"):
            per = np.linalg.norm(e[None] - g, axis=-1).max(axis=1)
        per[np.isnan(per)] = np.inf                               # a non-finite pose is infinitely wrong, never a match
        out["mssd"], out["mssd_sym"] = float(per.min()), int(per.argmin())
    if "mspd" in kinds:
        K = np.asarray(K, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            pe = (e @ K.T)[:, :2] / e[:, 2:3]
            pg = (g @ K.T)[..., :2] / g[..., 2:3]
            per = np.linalg.norm(pe[None] - pg, axis=-1).max(axis=1)
        per[(e[:, 2].min() <= 0) | (g[..., 2].min(axis=1) <= 0) | np.isnan(per)] = np.inf
        out["mspd"], out["mspd_sym"] = float(per.min()), int(per.argmin())
    if "add" in kinds:
        out["add"] = float(np.linalg.norm(e - (V @ Rg.T + tg), axis=-1).mean())
    if "adds" in kinds:
        Va = V if V_adds is None else np.asarray(V_adds, dtype=np.float64)
        out["adds"] = float(_nn_dist(Va @ Re.T + te, Va @ Rg.T + tg).mean())
    return out


def greedy_recalls(est, gts, targets, error_fn, limit_fn, n_thresholds):
    """The localization protocol on plain Python containers.  est: list of {"scene", "im", "obj", "score", "pose"}; gts:
    {(scene, im): [{"obj", "pose"}]}; targets: [(scene, im, obj, inst_count)]; error_fn(obj, pose_est, pose_gt, scene, im) -> error;
    limit_fn(obj, k) -> the limit at threshold k.  -> (recall per threshold, {obj: recall per threshold}, errors computed)."""
    hits, hits_obj, total_obj, seen = np.zeros(n_thresholds), {}, {}, []
    for scene, im, obj, count in targets:
        mine = [(i, e) for i, e in enumerate(est) if (e["scene"], e["im"], e["obj"]) == (scene, im, obj)]
        mine.sort(key=lambda ie: (-ie[1]["score"], ie[0]))
        mine = mine[:count]
        inst = [(j, g) for j, g in enumerate(gts.get((scene, im), [])) if g["obj"] == obj]
        err = {(i, j): error_fn(obj, e["pose"], g["pose"], scene, im) for i, e in mine for j, g in inst}
        seen += list(err.values())
        total_obj[obj] = total_obj.get(obj, 0) + count
        hits_obj.setdefault(obj, np.zeros(n_thresholds))
        for k in range(n_thresholds):
            used = set()
            for i, _e in mine:
                free = [(err[i, j], j) for j, _g in inst if j not in used and err[i, j] < limit_fn(obj, k)]
                if free:
                    used.add(min(free)[1])
                    hits[k] += 1
                    hits_obj[obj][k] += 1
    total = sum(t[3] for t in targets)
    return hits / total, {o: hits_obj[o] / total_obj[o] for o in hits_obj}, np.array(seen)


# ---- part 2: the kernel's arithmetic, float32 -------------------------------------------------------------------------------------
def compose32(Rg, tg, sym_R, sym_t):
    """Item 1: (S, 12) float32 = f32(R_gt R_s | R_gt t_s + t_gt), each entry ((a0 b0 + a1 b1) + a2 b2) [+ t] in float64."""
    A, t = np.asarray(Rg, dtype=F).astype(np.float64).reshape(3, 3), np.asarray(tg, dtype=F).astype(np.float64).reshape(3)
    B = np.asarray(sym_R, dtype=F).astype(np.float64).reshape(-1, 3, 3)
    b = np.asarray(sym_t, dtype=F).astype(np.float64).reshape(-1, 3)
    out = np.zeros((len(B), 12), dtype=F)
    for r in range(3):
        for c in range(3):
            out[:, 3 * r + c] = ((A[r, 0] * B[:, 0, c] + A[r, 1] * B[:, 1, c]) + A[r, 2] * B[:, 2, c]).astype(F)
        out[:, 9 + r] = (((A[r, 0] * b[:, 0] + A[r, 1] * b[:, 1]) + A[r, 2] * b[:, 2]) + t[r]).astype(F)
    return out


def apply32(T, V):
    """Item 2: T (..., 12) float32 maps, V (Nv, 3) float32 -> X, Y, Z of shape (..., Nv)."""
    T = np.asarray(T, dtype=F)[..., None]
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    return tuple(((T[..., 3 * r, :] * x + T[..., 3 * r + 1, :] * y) + T[..., 3 * r + 2, :] * z) + T[..., 9 + r, :] for r in range(3))


def _map12(R, t):
    return np.concatenate([np.asarray(R, dtype=F).reshape(9), np.asarray(t, dtype=F).reshape(3)])


def _nn_d2_f32(e, g):
    """min over the rows of g of the float32 squared distance in difference form, per row of e (float32 points)."""
    def d2(a, b):
        d = a - b
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    if len(g) <= BRUTE:
        return d2(e[:, None, :], g[None, :, :]).min(axis=1)
    # the float32 value is the true squared distance of the float32 points within a factor (1 +- 2^-21): the minimiser is among the
    # points whose true distance is within (1 + 1e-5) of the nearest one.  Take the 8 nearest; fall back to a ball query where the
    # 8th is still that close.
    from scipy.spatial import cKDTree

    tree = cKDTree(g.astype(np.float64))
    dist, idx = tree.query(e.astype(np.float64), k=8)
    out = d2(e[:, None, :], g[idx]).min(axis=1)
    for i in np.where(dist[:, -1] <= dist[:, 0] * (1 + 1e-5) + 1e-30)[0]:
        cand = tree.query_ball_point(e[i].astype(np.float64), dist[i, 0] * (1 + 1e-5) + 1e-30)
        out[i] = d2(e[i][None], g[cand]).min()
    return out


def errors32(V, sym_R, sym_t, Re, te, Rg, tg, fx=None, fy=None, kinds=("mssd", "mspd", "add", "adds"), V_adds=None):
    """One pair in the kernel's arithmetic.  V (Nv, 3) float32, sym_R (S, 9) / sym_t (S, 3) float32 (what ObjectModels uploads)."""
    V = np.asarray(V, dtype=F)
    out = {}
    E = _map12(Re, te)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Xe, Ye, Ze = apply32(E, V)
        if "mssd" in kinds or "mspd" in kinds:
            Xg, Yg, Zg = apply32(compose32(Rg, tg, sym_R, sym_t), V)                        # (S, Nv)
        if "mssd" in kinds:
            dx, dy, dz = Xe - Xg, Ye - Yg, Ze - Zg
            d2 = (dx * dx + dy * dy) + dz * dz
            per = np.sqrt(np.where(d2 == d2, d2, F(np.inf)).max(axis=1))            # a NaN squared distance counts as +inf
            out["mssd"], out["mssd_sym"] = per.min(), int(per.argmin())
        if "mspd" in kinds:
            fx, fy = F(fx), F(fy)
            rze, rzg = F(1) / Ze, F(1) / Zg
            du, dv = (fx * Xe) * rze - (fx * Xg) * rzg, (fy * Ye) * rze - (fy * Yg) * rzg
            d2 = du * du + dv * dv
            d2 = np.where(d2 == d2, d2, F(np.inf))
            d2 = np.where((Ze > 0)[None] & (Zg > 0), d2, F(np.inf))
            per = np.sqrt(d2.max(axis=1))
            out["mspd"], out["mspd_sym"] = per.min(), int(per.argmin())
        G = _map12(Rg, tg)
        if "add" in kinds:
            Xg, Yg, Zg = apply32(G, V)
            dx, dy, dz = Xe - Xg, Ye - Yg, Ze - Zg
            out["add"] = F(np.sqrt((dx * dx + dy * dy) + dz * dz).sum(dtype=np.float64) / len(V))
        if "adds" in kinds:
            Va = V if V_adds is None else np.asarray(V_adds, dtype=F)
            e, g = np.stack(apply32(E, Va), axis=1), np.stack(apply32(G, Va), axis=1)
            out["adds"] = F(np.sqrt(_nn_d2_f32(e, g)).sum(dtype=np.float64) / len(Va))
    return out


# ---- part 3: bounds ---------------------------------------------------------------------------------------------------------------
def max_norm(V, syms):
    """max over the vertices and symmetries of |x| and |S x| (float64)."""
    V, syms = np.asarray(V, dtype=np.float64), np.asarray(syms, dtype=np.float64)
    n = np.linalg.norm(V, axis=1).max()
    return float(n + np.linalg.norm(syms[:, :3, 3], axis=1).max())


def metric_bound(maxnorm, te, tg):
    """|err32 - err64| <= 16 2^-24 (max|x| + |t_est| + |t_gt|) for MSSD, ADD, ADD-S: every transformed coordinate is three products and
    three sums of magnitude <= M, i.e. <= 3 ulp(M); the difference, the squared norm and the root add fewer than that again."""
    return 16 * EPS * (maxnorm + float(np.linalg.norm(te)) + float(np.linalg.norm(tg)))


MSPD_C = 48


def mspd_bound(maxnorm, te, tg, f, z_min):
    """|mspd32 - mspd64| <= c 2^-24 (f M / z_min) (1 + M / z_min), M = max|x| + max(|t_est|, |t_gt|), f = max(fx, fy), z_min the
    smallest depth of any point under either pose, c = 48.  With e = 2^-24 and B = (f M / z_min)(1 + M / z_min):
      * a coordinate of the estimate's point: three products (relative e each, their magnitudes sum to <= sqrt(3)|x|) and three sums
        of partial results <= sqrt(3)|x| + |t|: error <= (sqrt(3) + 3 (sqrt(3) + 1)) e M < 7 e M since sqrt(3)|x| + |t| <= sqrt(3) M
        is pessimistic for both; the ground-truth side adds the rounding of the composed map's entries, sqrt(3) e |x| + e |g|:
        < 10 e M.  Take a = 10 for both.
      * u = (f X)(1 / Z) is three more roundings: |du| <= f (a e M / Z)(1 + |X| / Z) + 3 e f |X| / Z <= (a + 3) e B.
      * two sides and two image coordinates: the difference vector moves by <= 2 sqrt(2) (a + 3) e B < 37 e B; the subtraction, the
        squares, their sum and the root are relative 3 e of a distance <= 2 sqrt(2) f M / z_min: < 9 e B.  c = 48 covers 37 + 9.
      * the maximum over vertices and the minimum over symmetries move by at most the largest change of their arguments.
    The float64 oracle is given the float32 symmetry transforms the device holds, so their rounding is not part of the bound."""
    M = maxnorm + max(float(np.linalg.norm(te)), float(np.linalg.norm(tg)))
    return MSPD_C * EPS * (f * M / z_min) * (1 + M / z_min)


def min_depth(V, syms, Re, te, Rg, tg):
    V, syms = np.asarray(V, dtype=np.float64), np.asarray(syms, dtype=np.float64)
    ze = (V @ np.asarray(Re, dtype=np.float64)[2] + te[2]).min()
    sv = np.einsum("sij,nj->sni", syms[:, :3, :3], V) + syms[:, None, :3, 3]
    return float(min(ze, (sv @ np.asarray(Rg, dtype=np.float64)[2] + tg[2]).min()))


# ---- shared test inputs -----------------------------------------------------------------------------------------------------------
def random_rotation(rng, max_angle=math.pi):
    """A rotation by a uniform angle in [0, max_angle] about a uniform axis."""
    a = rng.normal(size=3)
    return axis_rotation(a / np.linalg.norm(a), rng.uniform(0, max_angle))


def cube_symmetries(half=1.0):
    """The 24 rotations of the cube (signed permutation matrices of determinant +1) as symmetries_discrete rows, identity left out."""
    import itertools

    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3))
            for r in range(3):
                R[r, perm[r]] = signs[r]
            if round(np.linalg.det(R)) == 1 and not np.array_equal(R, np.eye(3)):
                T = np.eye(4)
                T[:3, :3] = R
                out.append(T.reshape(16).tolist())
    return out


def mixed_inputs(seed=3, n_pairs=256):
    """The GPU suite's mixed call: a cube with its 24 symmetries, a 10 242-vertex sphere with a continuous symmetry (315 transforms) and
    a 30 000-vertex random mesh without symmetry; estimates around the ground truth at 1 mm / 1 degree (even pairs) and at 100 mm / up
    to 90 degrees (odd pairs); two cameras.  Every pose is float32-representable.  -> (objects for ObjectModels, pairs dict)."""
    import render_oracle as ro

    rng = np.random.default_rng(seed)
    cube = ro.cube(40.0)["vertices"]
    objects = {1: {"vertices": cube, "info": {"diameter": 80.0 * math.sqrt(3.0), "symmetries_discrete": cube_symmetries()}},
               2: {"vertices": ro.icosphere(5, 50.0)["vertices"],
                   "info": {"diameter": 100.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}},
               3: {"vertices": (rng.uniform(-1, 1, (30000, 3)) * [120.0, 80.0, 60.0]).astype(F), "info": {"diameter": 312.4}}}
    n_heavy = n_pairs * 7 // 64                                   # 28 of 256 for each of the two large objects
    ids = rng.permutation(np.array([1] * (n_pairs - 2 * n_heavy) + [2] * n_heavy + [3] * n_heavy))
    Ks = np.array([[[1066.778, 0, 312.9869], [0, 1067.487, 241.3109], [0, 0, 1]], [[572.4114, 0, 325.2611], [0, 573.57043, 242.049], [0, 0, 1]]])
    Rg, tg, Re, te = [], [], [], []
    for i in range(n_pairs):
        R, t = random_rotation(rng), np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(600, 1500)])
        ang, dist = (math.radians(1.0), 1.0) if i % 2 == 0 else (rng.uniform(0, math.pi / 2), 100.0)
        d = rng.normal(size=3)
        Rg.append(R)
        tg.append(t)
        Re.append(R @ random_rotation(rng, ang))
        te.append(t + dist * d / np.linalg.norm(d))
    f32 = lambda a: np.array(a).astype(F)                        # noqa: E731
    return objects, {"obj_ids": ids, "R_est": f32(Re), "t_est": f32(te), "R_gt": f32(Rg), "t_gt": f32(tg), "K": f32(Ks[np.arange(n_pairs) % 2])}
