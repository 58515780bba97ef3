"""Oracle of picopose_amd/model_info.py (a helper, not collected).

Part 1 generates the test meshes procedurally (no fixtures).  Part 2 restates the kernels' arithmetic (include/picopose_hip.h, "MODEL
INFO") in numpy float32, one ufunc per operation so that nothing is contracted — diameter32 and hausdorff32, which the kernels must
equal bit for bit — and the definitions in float64 (diameter64, hausdorff64).  Part 3 holds the float32 error bounds the GPU tests
assert.  Part 4 restates the host rule of find_symmetries with hausdorff32 in place of the kernel (find_symmetries_ref)."""
import math
from fractions import Fraction

import numpy as np

F = np.float32
EPS = 2.0 ** -24
SHIFT = (7.0, -3.0, 11.0)                                        # every symmetry mesh is translated by this, so that a centre bug shows


# ---- part 1: meshes ------------------------------------------------------------------------------------------------------------------
def _f32(v, shift=(0.0, 0.0, 0.0), R=None):
    v = np.asarray(v, dtype=np.float64)
    if R is not None:
        v = v @ np.asarray(R, dtype=np.float64).T
    return np.ascontiguousarray((v + np.asarray(shift, dtype=np.float64)).astype(F))


def box(sx, sy, sz, step=10.0, shift=(0.0, 0.0, 0.0), R=None):
    """The surface lattice of an sx x sy x sz box centred at the origin (every face gridded at `step`), rotated by R, then shifted."""
    ax = [np.linspace(-s / 2.0, s / 2.0, int(round(s / step)) + 1) for s in (sx, sy, sz)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    on = (np.abs(np.abs(g) - np.array([sx, sy, sz]) / 2.0) < 1e-9).any(axis=1)
    return _f32(g[on], shift, R)


def cube(side, shift=(0.0, 0.0, 0.0)):
    """The 8 corners of a cube of edge `side` centred at the origin, shifted."""
    h = side / 2.0
    return _f32([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], shift)


def prism(n, radius, height, shift=(0.0, 0.0, 0.0)):
    """The 2 n corners of a right prism over a regular n-gon (a corner on the +x axis), axis z, centred at the origin, shifted."""
    a = 2.0 * math.pi * np.arange(n) / n
    ring = np.stack([radius * np.cos(a), radius * np.sin(a)], axis=1)
    return _f32(np.concatenate([np.c_[ring, np.full(n, -height / 2.0)], np.c_[ring, np.full(n, height / 2.0)]]), shift)


def noisy(v, sigma, seed=0):
    return _f32(np.asarray(v, dtype=np.float64) + np.random.default_rng(seed).normal(0.0, sigma, np.shape(v)))


def box_diameter(sx, sy, sz):
    return math.sqrt(sx * sx + sy * sy + sz * sz)


def prism_diameter(n, radius, height):
    """The longest chord of the regular n-gon, 2 r sin(pi floor(n / 2) / n), against the height."""
    chord = 2.0 * radius * math.sin(math.pi * (n // 2) / n)
    return math.sqrt(chord * chord + height * height)


def generic_rotation():
    """A fixed rotation with no axis near a coordinate axis."""
    return rotation(np.array([0.36, -0.48, 0.8]), 1.1)


def rotation(axis, angle):
    x, y, z = (float(c) for c in axis)
    c, s = math.cos(angle), math.sin(angle)
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    a = np.array([x, y, z])
    return c * np.eye(3) + s * K + (1.0 - c) * np.outer(a, a)


# ---- part 2: the arithmetic ----------------------------------------------------------------------------------------------------------
def _d2(px, py, pz, qx, qy, qz):
    dx, dy, dz = px - qx, py - qy, pz - qz
    return (dx * dx + dy * dy) + dz * dz


def diameter32(v, rows=256):
    """Item 2: (d2max float32, (i, j)): the maximum over i < j of the float32 squared distance in difference form and the
    lexicographically lowest pair that attains it; one vertex: (0, (0, 0))."""
    v = np.asarray(v, dtype=F)
    best, pair = F(-1), (0, 0)
    n = len(v)
    for i0 in range(0, n, rows):
        a = v[i0:i0 + rows]
        d2 = _d2(a[:, None, 0], a[:, None, 1], a[:, None, 2], v[None, :, 0], v[None, :, 1], v[None, :, 2])
        d2[np.arange(n)[None, :] <= (i0 + np.arange(len(a)))[:, None]] = F(-1)
        k = int(np.argmax(d2))                                   # the first occurrence in row-major order: the lowest (i, j) of the block
        if d2.flat[k] > best:                                    # strict, blocks in ascending i: the lowest over all
            best, pair = d2.flat[k], (i0 + k // n, k % n)
    return (best, pair) if best >= 0 else (F(0), (0, 0))


def diameter64(v):
    """The largest vertex-to-vertex distance, brute force in float64."""
    v = np.asarray(v, dtype=np.float64)
    best = 0.0
    for i0 in range(0, len(v), 256):
        d = v[i0:i0 + 256, None, :] - v[None, :, :]
        best = max(best, float((d * d).sum(-1).max()))
    return math.sqrt(best)


def map12(T):
    """(C, 4, 4) float64 -> (C, 12) float32, R row-major then t, every entry rounded once."""
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)
    return np.concatenate([T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]], axis=1).astype(F)


def apply32(T, q):
    """Item 3: one 12-vector on (N, 3) float32 points -> X, Y, Z."""
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return tuple(((T[3 * r] * x + T[3 * r + 1] * y) + T[3 * r + 2] * z) + T[9 + r] for r in range(3))


def hausdorff32(full, query, T12):
    """Item 4: (C,) float32 = sqrt(max over the query points of min over the full set of d2(T x, y)) in the kernel's arithmetic."""
    full, query, T12 = np.asarray(full, dtype=F), np.asarray(query, dtype=F), np.asarray(T12, dtype=F).reshape(-1, 12)
    out = np.zeros(len(T12), dtype=F)
    for c, T in enumerate(T12):
        X, Y, Z = apply32(T, query)
        m = F(0)
        for i0 in range(0, len(query), 512):
            s = slice(i0, i0 + 512)
            d2 = _d2(X[s, None], Y[s, None], Z[s, None], full[None, :, 0], full[None, :, 1], full[None, :, 2])
            m = max(m, d2.min(axis=1).max())
        out[c] = np.sqrt(F(m))
    return out


def hausdorff64(full, query, T12):
    """The directed Hausdorff distance of the float32 points under the float32 maps, evaluated in float64."""
    full, query = np.asarray(full, dtype=np.float64), np.asarray(query, dtype=np.float64)
    out = np.zeros(len(T12))
    for c, T in enumerate(np.asarray(T12, dtype=np.float64).reshape(-1, 12)):
        p = query @ T[:9].reshape(3, 3).T + T[9:]
        m = 0.0
        for i0 in range(0, len(p), 512):
            d = p[i0:i0 + 512, None, :] - full[None, :, :]
            m = max(m, float((d * d).sum(-1).min(axis=1).max()))
        out[c] = math.sqrt(m)
    return out


def symmetric32(full, query, T):
    """max(h(T), h(T^-1)) of (C, 4, 4) float64 transforms, the inverse taken in float64 and rounded once."""
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)
    return np.maximum(hausdorff32(full, query, map12(T)), hausdorff32(full, query, map12(np.stack([inverse(t) for t in T]))))


# ---- part 3: bounds ------------------------------------------------------------------------------------------------------------------
DIAMETER_REL = 6 * EPS
"""model_diameter: every float32 squared distance is d2_true (1 + th), |th| <= (1 + e)^5 - 1 with e = 2^-24 (a difference, a square,
two sums: five roundings on the longest path).  The kernel's pair maximises the float32 value, so with D the true maximum
d2_true(pair) (1 + 5e') >= d2_32(pair) >= d2_32(true pair) >= D^2 (1 - 5e'), and diameter = d_true(pair) lies in
[D sqrt((1 - 5e') / (1 + 5e')), D]: 0 <= D - diameter <= 6 e D."""


def hausdorff_bound(query, T12, h64):
    """|h32 - h64| <= E + 4 e (h64 + E) + 2^-70, e = 2^-24, per candidate.  Derivation:
      * a coordinate of T x is three products and three sums: X = fl(fl(fl(p0 + p1) + p2) + t), p_k = fl(T_k x_k).  With
        P = |T0 x| + |T1 y| + |T2 z| the products err by <= e P in all, and each sum by e times its own magnitude, <= P, P and P + |t|:
        |X32 - X| <= e (4 P + |t|) (1 + 8 e).  E is the Euclidean norm of the three coordinate bounds, each taken at the query point
        that maximises it: every transformed point is displaced by at most E.
      * a directed Hausdorff distance moves by at most the largest displacement of its points: |H(displaced) - h64| <= E.
      * the float32 squared distance of two float32 points is the true one times (1 + th), |th| <= (1 + e)^5 - 1 (DIAMETER_REL's
        note); minimum, maximum and the correctly rounded square root are monotone, so h32 = H(displaced) sqrt(1 + th') (1 + e''):
        within (2.5 + 1) e of it, 4 e covering the second-order terms.
      * a square below 2^-126 loses relative accuracy to underflow; that is a distance below 2^-63 and an absolute error below 2^-70."""
    q = np.abs(np.asarray(query, dtype=np.float64))
    T = np.abs(np.asarray(T12, dtype=np.float64).reshape(-1, 12))
    P = np.stack([(q[None] * T[:, None, 3 * r:3 * r + 3]).sum(-1).max(axis=1) for r in range(3)], axis=1)      # (C, 3)
    E = np.linalg.norm(EPS * (4.0 * P + T[:, 9:]) * (1 + 8 * EPS), axis=1)
    return E + 4 * EPS * (np.asarray(h64) + E) + 2.0 ** -70


# ---- part 4: the host rule of find_symmetries ----------------------------------------------------------------------------------------
NEAR = 1e-6


def inverse(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def product(A, B):
    """Every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3: the stated order of the rule's compose."""
    return np.stack([((A[r, 0] * B[0] + A[r, 1] * B[1]) + A[r, 2] * B[2]) + A[r, 3] * B[3] for r in range(4)])


def about(axis, angle, centre):
    T = np.eye(4)
    T[:3, :3] = rotation(axis, angle)
    T[:3, 3] = centre - T[:3, :3] @ centre
    return T


def fractions(max_order, continuous_steps):
    cont = [Fraction(k, continuous_steps) for k in range(1, continuous_steps)]
    seen = []
    for f in [Fraction(k, n) for n in range(2, max_order + 1) for k in range(1, n)] + cont:
        if f not in seen:
            seen.append(f)
    return sorted(seen), cont


def axes_ref(v):
    v = np.asarray(v, dtype=np.float64)
    d = v - v.mean(axis=0)
    _, vec = np.linalg.eigh(d.T @ d / len(v))
    out = []
    for a in [np.eye(3)[0], np.eye(3)[1], np.eye(3)[2], vec[:, 0], vec[:, 1], vec[:, 2]]:
        a = a / np.linalg.norm(a)
        if a[int(np.argmax(np.abs(a)))] < 0:
            a = -a
        if all(min(np.abs(a - b).max(), np.abs(a + b).max()) > NEAR for b in out):
            out.append(a)
    return out


def _close(T, pool):
    return any(np.abs(T - E).max() <= NEAR for E in pool)


def _coset(T, kept, cont_axes, centre):
    """T = C E with C a rotation about a continuous axis through the centre, E the identity or a kept element."""
    for E in [np.eye(4)] + kept:
        M = product(T, inverse(E))
        for a in cont_axes:
            if np.abs(M[:3, :3] @ a - a).max() <= NEAR and np.abs(M[:3, :3] @ centre + M[:3, 3] - centre).max() <= NEAR:
                return True
    return False


def find_symmetries_ref(v, tol="bop", diameter=None, centre=None, max_order=12, continuous_steps=72, max_points=4096, max_rounds=4,
                        max_elements=120, measure=None):
    """The rule of model_info.find_symmetries, steps 1-6, with hausdorff32 as the measurement (or `measure(transforms) -> deviations`)."""
    v = np.asarray(v, dtype=F)
    if tol == "bop":
        if diameter is None:
            _, (i, j) = diameter32(v)
            diameter = float(np.linalg.norm(v[i].astype(np.float64) - v[j].astype(np.float64)))
        tol = max(15.0, 0.1 * diameter)
    q = v if max_points is None else v[::-(-len(v) // max_points)]
    measure = measure or (lambda T: symmetric32(v, q, T))
    v64 = v.astype(np.float64)
    centre = (v64.min(axis=0) + v64.max(axis=0)) / 2.0 if centre is None else np.asarray(centre, dtype=np.float64)
    axes = axes_ref(v)
    fr, cont = fractions(max_order, continuous_steps)
    cands = [[about(a, 2.0 * math.pi * float(f), centre) for f in fr] for a in axes]
    dev = np.asarray(measure(np.stack([T for row in cands for T in row])), dtype=np.float64).reshape(len(axes), len(fr))
    measured = len(axes) * len(fr)
    continuous = [all(dev[a, fr.index(f)] <= tol for f in cont) for a in range(len(axes))]
    cont_axes = [axes[a] for a in range(len(axes)) if continuous[a]]
    cont_dev = [max(float(dev[a, fr.index(f)]) for f in cont) for a in range(len(axes)) if continuous[a]]
    kept, kept_dev, rejected = [], [], []
    for a in range(len(axes)):
        if continuous[a]:
            continue
        for i, T in enumerate(cands[a]):
            if dev[a, i] > tol:
                rejected.append(T)
            elif len(kept) < max_elements and not _close(T, kept) and not _coset(T, kept, cont_axes, centre):
                kept.append(T)
                kept_dev.append(float(dev[a, i]))
    for _ in range(max_rounds):
        if not kept or len(kept) >= max_elements:
            break
        new = []
        for A in kept:
            for B in kept:
                T = product(A, B)
                if np.abs(T - np.eye(4)).max() <= NEAR or _close(T, kept) or _close(T, rejected) or _close(T, new):
                    continue
                if not _coset(T, kept, cont_axes, centre):
                    new.append(T)
        if not new:
            break
        d = np.asarray(measure(np.stack(new)), dtype=np.float64)
        measured += len(new)
        before = len(kept)
        for T, e in zip(new, d):
            if e > tol:
                rejected.append(T)
            elif len(kept) < max_elements and not _coset(T, kept, cont_axes, centre):
                kept.append(T)
                kept_dev.append(float(e))
        if len(kept) == before:
            break
    return {"symmetries_discrete": [T.reshape(16).tolist() for T in kept],
            "symmetries_continuous": [{"axis": a.tolist(), "offset": centre.tolist()} for a in cont_axes],
            "candidates": measured, "deviation": kept_dev + cont_dev}


# ---- the symmetry cases of the GPU suite -----------------------------------------------------------------------------------------------
def symmetry_cases():
    """{name: (vertices, tol, expected (discrete, continuous) counts or None)}.  The counts are what find_symmetries_ref yields (confirmed
    on the CPU by tests/test_model_info_cpu.py); every mesh is shifted by SHIFT."""
    return {
        "box": (box(20, 30, 50, shift=SHIFT), 1e-3, (3, 0)),                                      # D2
        "cube": (cube(40, SHIFT), 1e-3, (23, 0)),                                                   # needs the closure rounds
        # the rule's centre is the centre of the vertex BOX, which for an odd n-gon is not on the prism's axis: only the flip about x,
        # whose axis passes through both, is found there; with the true centre handed in the whole dihedral group is
        "prism5": (prism(5, 30, 40, SHIFT), 1e-3, (1, 0)),
        "prism7": (prism(7, 30, 40, SHIFT), 1e-3, (1, 0)),
        "prism72": (prism(72, 30, 40, SHIFT), 1e-3, (1, 1)),                                        # continuous z, one flip modulo the axis
        "box_rotated": (box(20, 30, 50, shift=SHIFT, R=generic_rotation()), 1e-3, (3, 0)),          # through the principal axes only
        "box_noisy": (noisy(box(20, 30, 50, shift=SHIFT), 2.0), 1e-3, (0, 0)),
        "box_bop": (box(20, 30, 50, shift=SHIFT), "bop", None),                                     # whatever the rule yields: > 3
    }


CENTRED_PRISMS = {"prism5": (9, 0), "prism7": (13, 0)}            # the same prisms with centre=SHIFT: D5 and D7
