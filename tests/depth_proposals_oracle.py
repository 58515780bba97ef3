"""numpy restatement of "DEPTH PROPOSALS" (include/picopose_hip.h; csrc/pp_depth_proposals.hip), and the scenes its tests use.

Every float32 expression that decides a comparison is evaluated on numpy float32 arrays in the header's order (numpy rounds each
operation once and never contracts), so the integer outputs — scores, winner, labels, records, run ends — must equal the device's bit
for bit.  The refit is numpy.linalg.eigh in float64; the components are scipy's connected_components on the explicit 4-neighbour
edge list, relabelled to the smallest pixel index; the run lengths are scene_gt.rle_from_mask's."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from picopose_amd.provider.test_batch import rle_counts
from picopose_amd.scene_gt import rle_from_mask

F = np.float32
MIN_CROSS2 = F(1.0)         # PP_PLANE_MIN_CROSS2
M32 = 0xFFFFFFFF


def aug_mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def aug_hash(seed, a, b):
    return aug_mix(seed ^ aug_mix(a ^ aug_mix((b + 0x9E3779B9) & M32)))


def valid(depth):
    with np.errstate(invalid="ignore"):
        return (depth > 0) & (depth < np.inf)


def points(depth, cam):
    """(H, W) float32 and (fx, fy, cx, cy) -> X, Y, Z (H, W) float32: THE POINT, NaN where the pixel is invalid."""
    H, W = depth.shape
    fx, fy, cx, cy = (F(v) for v in cam)
    u, v = np.arange(W, dtype=F)[None, :], np.arange(H, dtype=F)[:, None]
    z = np.where(valid(depth), depth, F(np.nan)).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        X = ((u - cx) * z) / fx
        Y = ((v - cy) * z) / fy
    assert X.dtype == F and Y.dtype == F
    return X, Y, z


def height(plane, X, Y, Z):
    """THE HEIGHT: ((nx X + ny Y) + nz Z) + d in float32."""
    nx, ny, nz, d = (F(v) for v in plane)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((nx * X + ny * Y) + nz * Z) + d


def hypothesis(depth, P, seed, b, h):
    """-> (plane (4,) float32, p0 (3,) float32) or None for a dead hypothesis."""
    H, W = depth.shape
    X, Y, Z = P
    p = []
    for k in range(3):
        i = (aug_hash(seed, b, 3 * h + k) * (H * W)) >> 32
        v, u = divmod(i, W)
        if not valid(depth[v, u]):
            return None
        p.append(np.array([X[v, u], Y[v, u], Z[v, u]], dtype=F))
    with np.errstate(over="ignore", invalid="ignore"):
        a, e = p[1] - p[0], p[2] - p[0]
        c = np.array([a[1] * e[2] - a[2] * e[1], a[2] * e[0] - a[0] * e[2], a[0] * e[1] - a[1] * e[0]], dtype=F)
        len2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        if not (len2 > MIN_CROSS2 and len2 < np.inf):
            return None
        inv = F(1.0) / np.sqrt(len2)
        n = c * inv
        d = -((n[0] * p[0][0] + n[1] * p[0][1]) + n[2] * p[0][2])
    assert n.dtype == F and type(d) is F and type(inv) is F
    return np.array([n[0], n[1], n[2], d], dtype=F), p[0]


def plane(depth, cam, b=0, n_hyp=256, seed=0, tau=5.0, min_inliers=1000):
    """One image -> {"scores" (n_hyp,), "winner", "count", "has_plane", "consensus" (H, W) bool, "refit_count", "plane64", "plane"}."""
    P = points(depth, cam)
    scores = np.zeros(n_hyp, np.int64)
    hyps = [hypothesis(depth, P, seed, b, h) for h in range(n_hyp)]
    for h, hyp in enumerate(hyps):
        if hyp is not None:
            with np.errstate(invalid="ignore"):
                scores[h] = int((np.abs(height(hyp[0], *P)) <= F(tau)).sum())
    winner = int(np.argmax(scores))                                 # (the first of the largest)
    count = int(scores[winner])
    out = {"scores": scores, "winner": winner, "count": count, "has_plane": count >= min_inliers, "consensus": np.zeros(depth.shape, bool),
           "refit_count": 0, "plane64": np.zeros(4), "plane": np.zeros(4, F)}
    if out["has_plane"]:
        pl, p0 = hyps[winner]
        with np.errstate(invalid="ignore"):
            cons = np.abs(height(pl, *P)) <= F(tau)
        out["consensus"], out["refit_count"] = cons, int(cons.sum())
        out["plane64"] = eigh_fit(np.stack([a[cons] for a in P], axis=1).astype(np.float64))
        out["plane"] = out["plane64"].astype(F)
    return out


def eigh_fit(pts):
    """(N, 3) float64 -> (nx, ny, nz, d) float64: the least-squares plane, d >= 0."""
    c = pts.mean(axis=0)
    q = pts - c
    w, v = np.linalg.eigh(q.T @ q / len(pts))
    n = v[:, 0] / np.linalg.norm(v[:, 0])
    d = -float(n @ c)
    if d < 0:
        n, d = -n, -d
    return np.array([n[0], n[1], n[2], d])


def foreground(depth, cam, plane32, has_plane, min_height=10.0, max_height=400.0, max_range=3000.0):
    X, Y, Z = points(depth, cam)
    with np.errstate(invalid="ignore"):
        fg = valid(depth) & (Z <= F(max_range))
        if has_plane:
            s = height(plane32, X, Y, Z)
            fg &= (s > F(min_height)) & (s < F(max_height))
    return fg


def labels(depth, fg, max_step=15.0):
    """(H, W) float32 and the foreground -> (H, W) int32: -1, or the smallest row-major index of the pixel's component."""
    H, W = depth.shape
    idx = np.arange(H * W).reshape(H, W)
    z = depth.astype(F)
    rows, cols = [], []
    with np.errstate(invalid="ignore"):
        for p, q in (((slice(None), slice(1, None)), (slice(None), slice(None, -1))), ((slice(1, None), slice(None)), (slice(None, -1), slice(None)))):
            link = fg[p] & fg[q] & (np.abs(z[p] - z[q]) <= F(max_step))
            rows.append(idx[p][link])
            cols.append(idx[q][link])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(H * W, H * W))
    n, comp = connected_components(graph, directed=False)
    first = np.full(n, H * W, np.int64)
    np.minimum.at(first, comp, np.arange(H * W))
    return np.where(fg.ravel(), first[comp], -1).astype(np.int32).reshape(H, W)


def stats(lab):
    """(H, W) labels -> {root: (area, xmin, ymin, xmax, ymax, border)}."""
    H, W = lab.shape
    out = {}
    for root in np.unique(lab[lab >= 0]):
        ys, xs = np.nonzero(lab == root)
        border = int(xs.min() == 0 or ys.min() == 0 or xs.max() == W - 1 or ys.max() == H - 1)
        out[int(root)] = (len(ys), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()), border)
    return out


def qualifying(st, min_area, max_area, drop_border):
    """The records (root, area, xmin, ymin, xmax, ymax, border) that qualify, area descending and then root ascending."""
    rows = [(r,) + v for r, v in st.items() if min_area <= v[0] <= max_area and not (drop_border and v[5])]
    return sorted(rows, key=lambda t: (-t[1], t[0]))


def run_ends(lab, root):
    return np.cumsum(rle_counts(rle_from_mask(lab == root)))


def proposals(depth, cam, n_hyp=256, seed=0, tau=5.0, min_inliers=1000, min_height=10.0, max_height=400.0, max_range=3000.0,
              max_step=15.0, min_area_px=200, max_area_frac=0.5, drop_border=False, max_proposals=200):
    """All four stages on one image: what depth_proposals must return (with the oracle's own plane)."""
    H, W = depth.shape
    pl = plane(depth, cam, 0, n_hyp, seed, tau, min_inliers)
    lab = labels(depth, foreground(depth, cam, pl["plane"], pl["has_plane"], min_height, max_height, max_range), max_step)
    rows = qualifying(stats(lab), min_area_px, int(max_area_frac * H * W), drop_border)[:max_proposals]
    return [{"segmentation": rle_from_mask(lab == r[0]), "bbox": [r[2], r[3], r[4] - r[2] + 1, r[5] - r[3] + 1], "area": r[1]} for r in rows], pl, lab


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
FAR = F(9000.0)             # beyond max_range: background
NEAR = F(1000.0)
LABEL_SIZES = ((45, 70), (96, 80), (1, 130), (130, 1))


def serpentine(H, W):
    """A one-pixel-wide path: the even rows in full, joined alternately at the right and the left end."""
    m = np.zeros((H, W), bool)
    m[::2] = True
    for y in range(1, H, 2):
        m[y, W - 1 if (y // 2) % 2 == 0 else 0] = True
    return m


def comb(H, W):
    m = np.zeros((H, W), bool)
    m[0] = True
    m[:, ::2] = True
    m[H - 1, :] = False
    return m


def checkerboard(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy + xx) % 2 == 0


def last_pixel(H, W):
    """Blobs, one of which ends in the frame's last pixel; pixel 0 is set as well (a leading zero run)."""
    m = np.zeros((H, W), bool)
    m[max(H - 7, 0):, max(W - 5, 0):] = True
    m[H - 1, : max(W - 9, 1)] = True
    m[0, 0] = True
    m[H // 3: H // 3 + 4, W // 4: W // 4 + 9] = True
    return m


def depth_of(mask, rng=None):
    """Foreground at NEAR with a gentle ramp (far below max_step per pixel), background beyond the range."""
    H, W = mask.shape
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where(mask, NEAR + F(0.25) * (xx % 7).astype(F) + F(0.5) * (yy % 5).astype(F), FAR).astype(F)


def step_frame(H, W, max_step=15.0):
    """Four bands of two regions that touch: a step of exactly max_step (joined), the next float32 above it (split) — both at a
    depth whose float32 spacing shows the difference exactly — and the same pair at a metre, where the split step is max_step plus
    one spacing of the farther depth."""
    if W < 4 <= H:                                                  # a frame one pixel wide: the same, transposed
        return np.ascontiguousarray(step_frame(W, H, max_step).T)
    d = np.full((H, W), FAR, F)
    hb, wb = max(H // 4, 1), max(W // 2, 1)
    s = F(max_step)
    pairs = [(F(0.5), F(0.5) + s), (F(0.5), np.nextafter(F(0.5) + s, F(np.inf))), (NEAR, NEAR + s), (NEAR, np.nextafter(NEAR + s, F(np.inf)))]
    assert pairs[0][1] - pairs[0][0] == s and pairs[1][1] - pairs[1][0] == np.nextafter(s, F(np.inf)) and pairs[3][1] - pairs[3][0] > s
    for k, (a, b) in enumerate(pairs):
        if H >= 4:
            rows = slice(k * hb, (k + 1) * hb - 1)                  # (one background row between the bands)
            d[rows, :wb], d[rows, wb:] = a, b
        else:                                                       # a frame too low for bands: the pairs side by side
            w4 = max(W // 4, 2)
            d[:, k * w4: k * w4 + w4 // 2], d[:, k * w4 + w4 // 2: (k + 1) * w4 - 1] = a, b
    return d


def holes_frame(H, W, seed):
    """All foreground but for zeros, NaNs, infinities and negative depths sprinkled over it."""
    rng = np.random.default_rng(seed)
    d = depth_of(np.ones((H, W), bool))
    r = rng.random((H, W))
    d[r < 0.08] = 0
    d[(r >= 0.08) & (r < 0.16)] = np.nan
    d[(r >= 0.16) & (r < 0.20)] = np.inf
    d[(r >= 0.20) & (r < 0.24)] = -5.0
    return d


def label_frames(H, W):
    """name -> (H, W) float32 depth: the frames the labels are held to (no plane: the range test alone decides the foreground)."""
    return {"serpentine": depth_of(serpentine(H, W)), "comb": depth_of(comb(H, W)), "checkerboard": depth_of(checkerboard(H, W)),
            "full": depth_of(np.ones((H, W), bool)), "empty": depth_of(np.zeros((H, W), bool)), "last_pixel": depth_of(last_pixel(H, W)),
            "steps": step_frame(H, W), "holes": holes_frame(H, W, H * 1000 + W)}


def big_frame():
    """One 480 x 640 frame: a serpentine over the upper part, a comb, a checkerboard patch, a stepped pair and holes below it."""
    H, W = 480, 640
    d = np.full((H, W), FAR, F)
    d[:200] = depth_of(serpentine(200, W))
    d[210:330, :300] = depth_of(comb(120, 300))
    d[210:330, 310:] = depth_of(checkerboard(120, 330))
    d[340:400] = step_frame(60, W)
    d[410:] = holes_frame(70, W, 5)
    return d


def camera(H, W):
    f = 0.9 * max(H, W)
    return np.array([f, f * 1.01, (W - 1) / 2.0, (H - 1) / 2.0], F)


def table_scene(H, W, rects, normal=(0.12, -0.42, -0.9), dist=800.0, invalid=0.0, seed=0, keep_rects=False):
    """An analytic tilted plane (unit normal towards the camera, `dist` mm from it) with rectangles raised over it:
    rects = [(y0, y1, x0, x1, height_mm)], inclusive pixel bounds.  invalid: the fraction of pixels set to 0 / NaN (keep_rects: only
    off the rectangles).  -> (depth (H, W) float32, cam (4,) float32, masks: one (H, W) bool per rectangle)."""
    cam = camera(H, W)
    n = np.asarray(normal, np.float64)
    n /= np.linalg.norm(n)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(u - float(cam[2])) / float(cam[0]), (v - float(cam[3])) / float(cam[1]), np.ones_like(u)], axis=-1)
    nr = ray @ n                                                    # < 0: the plane faces the camera
    raise_by = np.zeros((H, W))
    masks = []
    for y0, y1, x0, x1, h in rects:
        m = np.zeros((H, W), bool)
        m[y0:y1 + 1, x0:x1 + 1] = True
        raise_by[m] = h
        masks.append(m)
    depth = (-(dist - raise_by) / nr).astype(F)                     # n . p + (dist - h) = 0
    if invalid:
        rng = np.random.default_rng(seed)
        r = rng.random((H, W))
        if keep_rects:
            r[raise_by > 0] = 1.0
        depth[r < invalid / 2] = 0
        depth[(r >= invalid / 2) & (r < invalid)] = np.nan
    return depth, cam, masks


# the end-to-end scene on the 45 x 70 frame: five rectangles raised 50-120 mm; A and B touch at different heights, E is below 200 px
E2E_RECTS = ((2, 17, 3, 22, 60.0), (2, 16, 23, 38, 110.0), (24, 40, 5, 19, 80.0), (22, 42, 30, 41, 120.0), (25, 34, 55, 64, 50.0))


def e2e_scene():
    return table_scene(45, 70, E2E_RECTS, invalid=0.1, seed=3, keep_rects=True)


def roof_scene(H=48, W=64):
    """Two planes that are mirror images about the frame's vertical centre line (cx = (W - 1) / 2): the hypotheses of the left half
    and those of the right half reach the same score.  -> (depth, cam)."""
    cam = camera(H, W)
    u = np.arange(W, dtype=np.float64)
    xr = np.abs(u - float(cam[2])) / float(cam[0])
    z = 800.0 / (1.0 + 0.6 * xr)                                    # z + 0.6 |X| = 800 on either side
    return np.broadcast_to(z.astype(F), (H, W)).copy(), cam
