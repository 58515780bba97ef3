"""Numpy float64 statement of the proposal labelling (TEST INFRASTRUCTURE, not collected): include/picopose_hip.h, PROPOSAL LABELLING,
and picopose_amd/proposals.py restated from their definitions.  It imports nothing from the package: normalise, cosine, top-k mean,
both arg-max rules, bit packing and intersections from a dense decode of the RLE, greedy NMS by brute force, the pipeline of
label_proposals after the descriptors, the error bound of `score`, and the seeded inputs the CPU and GPU tests share.

err_bound(C), derived from the kernel's stated orders; u = 2^-24, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., Lemma 3.1 and (3.5)).  The raw rows q, d are fp32 numbers and exact inputs of both sides.

1. Normalisation (pp_descriptor_normalize, THE ROW ORDER).  ss = sum x_i^2 over C non-negative terms, each entering through one fma
   and at most (C - 1) further additions on its way through the lane chain and the butterfly: any order of C terms obeys
   fl(ss) = ss (1 + t), |t| <= gamma(C) (the stated tree is shallower, ceil(C / 64) + 6 roundings; gamma(C) covers it for
   C >= 8, the smallest C used).  n = sqrtf(fl(ss)) and x_i / n: each at most one ulp = 2 u relative (they are correctly rounded,
   u, with hipcc's defaults; 2 u does not lean on the flag).  sqrt halves t.  So  xh_i = (x_i / ||x||) (1 + e_i),
   |e_i| <= delta(C) = gamma(C) / 2 + 4 u  (+ second order, point 4).  The max(., eps) never acts on the test's rows.
2. Dot product (pp_proposal_match, THE DOT ORDER): C products, each entering through one fma, summed in a fixed tree; for ANY
   order |fl(qh . dh) - qh . dh| <= gamma(C) sum |qh_i dh_i| <= gamma(C) ||qh|| ||dh|| <= gamma(C) (1 + delta)^2.
   The rows are unit vectors up to delta:  |qh . dh - (q . d) / (||q|| ||d||)| <= ((1 + delta)^2 - 1) sum |q_i d_i| / (||q|| ||d||)
   <= 2 delta + delta^2 (Cauchy-Schwarz).  A cosine therefore errs by at most  e_cos = gamma(C) + 2 delta(C)  (+ second order).
3. Top-k mean: the k <= 8 largest cosines added largest first (k - 1 additions) and one division: relative gamma(k) of
   sum |c| <= k max |c|, i.e. at most gamma(8) (1 + e_cos) on the mean.  Selecting the k largest of PERTURBED cosines instead of
   the exact ones moves the mean by at most e_cos: the sorted values of two vectors that differ by at most e_cos entry-wise differ by
   at most e_cos rank by rank (Weyl's inequality for order statistics).
4. Second-order terms (delta^2, gamma delta) are below 1e-3 of the total for C <= 1024: one factor 1.01.
       err_bound(C) = 1.01 (gamma(C) + 2 delta(C) + gamma(8)) = 1.01 (2 gamma(C) + 8 u + gamma(8)),
   1.243e-4 at C = 1024, i.e. 1.01 (C + 8) 2^-23.  Nothing in it was read off the kernel's output.
The float64 side's own error (C 2^-53) is nine orders below and not counted.

Labels and views are compared only where the float64 margin to the runner-up exceeds 2 err_bound (each side of the comparison may
move by err_bound); `undecided` counts what that leaves out and the tests cap it."""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def err_bound(C):
    return 1.01 * (2.0 * gamma(C) + 8.0 * U + gamma(8))


def normalize(x, eps=1e-12):
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), eps)


def match(query, bank, offsets, topk, unit_bank=False):
    """Raw fp32 rows -> dict(score (P, O), view (P, O), label (P,), best (P,), label_margin (P,), view_margin (P, O)), float64.
    unit_bank: the bank rows are taken as they are (the device's own unit rows)."""
    q = normalize(query)
    d = np.asarray(bank, np.float64) if unit_bank else normalize(bank)
    cos = q @ d.T
    P, O = q.shape[0], len(offsets) - 1
    score, view, vmargin = np.zeros((P, O)), np.zeros((P, O), np.int64), np.full((P, O), np.inf)
    for o in range(O):
        c = cos[:, offsets[o]:offsets[o + 1]]
        s = -np.sort(-c, axis=1)
        k = min(topk, c.shape[1])
        score[:, o] = s[:, :k].sum(1) / k
        view[:, o] = np.argmax(c, axis=1)                      # numpy's argmax returns the first of equal maxima
        if c.shape[1] > 1:
            vmargin[:, o] = s[:, 0] - s[:, 1]
    label = np.argmax(score, axis=1)
    best = score[np.arange(P), label]
    lmargin = np.full(P, np.inf)
    if O > 1:
        s = -np.sort(-score, axis=1)
        lmargin = s[:, 0] - s[:, 1]
    return {"score": score, "view": view, "label": label, "best": best, "label_margin": lmargin, "view_margin": vmargin}


def undecided(m, C):
    """-> (proposals whose label, (proposal, object) cells whose view) the bound cannot decide."""
    b = 2.0 * err_bound(C)
    return int((m["label_margin"] <= b).sum()), int((m["view_margin"] <= b).sum())


# ---- masks -------------------------------------------------------------------------------------------------------------------------

def rle_of(mask):
    """(h, w) binary mask -> uncompressed COCO RLE (column-major runs, the first run counts zeros and may be 0)."""
    flat = np.asarray(mask).astype(np.int8).ravel(order="F")
    bounds = np.concatenate(([0], np.nonzero(np.diff(flat))[0] + 1, [flat.size]))
    counts = np.diff(bounds).tolist()
    return {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": ([0] + counts) if flat[0] else counts}


def dense(segmentation):
    """Uncompressed COCO RLE -> the column-major pixel vector (h * w,) of 0 / 1."""
    counts = np.asarray(segmentation["counts"], np.int64)
    return np.repeat(np.arange(len(counts)) & 1, counts).astype(np.uint8)


def pack_bits(segmentations):
    """-> (bits (n, ceil(hw / 32)) uint32, area (n,) int32): bit i of word w = column-major pixel 32 w + i."""
    rows = []
    for seg in segmentations:
        flat = dense(seg)
        pad = np.concatenate((flat, np.zeros(-len(flat) % 32, np.uint8))).reshape(-1, 32).astype(np.uint64)
        rows.append((pad << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32))
    return np.stack(rows), np.array([int(dense(s).sum()) for s in segmentations], np.int32)


def intersections(segmentations):
    m = np.stack([dense(s) for s in segmentations]).astype(np.int64)
    return (m @ m.T).astype(np.int32)


def nms(scores, labels, inter, area, iou, per_object=True):
    """Greedy NMS by brute force: repeatedly take the best remaining proposal (lowest index among equal scores) and strike out
    every remaining one that overlaps it (per_object: and shares its label) with IoU > iou."""
    scores = np.asarray(scores, np.float64)
    alive = list(range(len(scores)))
    kept = []
    while alive:
        i = min(alive, key=lambda a: (-scores[a], a))
        kept.append(i)
        alive.remove(i)
        for j in list(alive):
            if per_object and labels[i] != labels[j]:
                continue
            union = int(area[i]) + int(area[j]) - int(inter[i][j])
            if union > 0 and float(inter[i][j]) / float(union) > iou:
                alive.remove(j)
    return kept


def label_pipeline(desc, bank_unit, offsets, obj_ids, segmentations, topk=5, min_score=0.5, max_detections=100, nms_iou=0.25):
    """label_proposals after the descriptors: match (the device's unit bank rows taken as they are), confidence cut, cap, NMS
    -> list of (proposal index, object id, score, view), best first."""
    m = match(desc, bank_unit, offsets, topk, unit_bank=True)
    order = sorted(range(len(desc)), key=lambda a: (-m["best"][a], a))
    cand = [a for a in order if m["best"][a] > min_score][:max_detections]
    if not cand:
        return []
    segs = [segmentations[a] for a in cand]
    area = pack_bits(segs)[1]
    kept = nms(m["best"][cand], m["label"][cand], intersections(segs), area, nms_iou)
    return [(cand[k], obj_ids[int(m["label"][cand[k]])], float(m["best"][cand[k]]), int(m["view"][cand[k], m["label"][cand[k]]])) for k in kept]


def mask_box(mask):
    ys, xs = np.nonzero(mask)
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


# ---- seeded inputs shared by the CPU and GPU tests -------------------------------------------------------------------------------------
P_SET, T_SET, C_SET, K_SET = (1, 17, 33), ((1,), (1, 4, 7), (5, 5, 9)), (8, 384, 1024), (1, 5)
SEED = 2                # fixed: the float64 side alone stays inside the cap for every case (tests/test_proposals_cpu.py asserts it;
UNDECIDED_CAP = 0.10    # of the seeds 0..39 thirty do, and seed 2 still leaves some comparisons out, so that path runs)


def offsets_of(T):
    return np.concatenate(([0], np.cumsum(T))).astype(np.int32)


def random_set(P, T, C, seed=SEED):
    """Gaussian rows: -> (query (P, C), bank (sum T, C)) fp32."""
    rng = np.random.default_rng([seed, P, sum(T), len(T), C])
    return rng.standard_normal((P, C)).astype(np.float32), rng.standard_normal((sum(T), C)).astype(np.float32)


def planted_set(P, T, C, seed=SEED):
    """Objects with orthogonal centres of norm sqrt(C) (C >= len(T)), templates = centre + 0.3 N(0, 1) (the views of one object
    resemble each other), every query = one template + 10 % noise (0.1 N(0, 1) on rows of unit variance).
    -> (query, bank, planted object (P,), planted view (P,))."""
    rng = np.random.default_rng([seed, P, sum(T), len(T), C, 1])
    centres = np.linalg.qr(rng.standard_normal((C, len(T))))[0].T * np.sqrt(C)
    bank = np.concatenate([centres[o] + 0.3 * rng.standard_normal((t, C)) for o, t in enumerate(T)]).astype(np.float32)
    obj = rng.integers(0, len(T), P)
    view = np.array([rng.integers(0, T[o]) for o in obj])
    off = offsets_of(T)
    query = (bank[off[obj] + view] + 0.1 * rng.standard_normal((P, C))).astype(np.float32)
    return query, bank, obj, view


def mask_set(H, W, n, seed=SEED):
    """n masks of an (H, W) frame: empty, full, a single pixel, the first pixel (column-major) alone — no leading zero run —, a
    mask whose first pixel is clear next to a set one, the last pixel, then random ones of mixed density; cycled up to n."""
    rng = np.random.default_rng([seed, H, W, n])
    kinds = []
    z = lambda: np.zeros((H, W), np.uint8)  # noqa: E731
    kinds.append(z())
    kinds.append(np.ones((H, W), np.uint8))
    m = z(); m[H // 2, W // 3] = 1; kinds.append(m)  # noqa: E702
    m = z(); m[0, 0] = 1; kinds.append(m)  # noqa: E702
    m = z(); m[1 % H, 0] = 1; m[H - 1, W - 1] = 1; kinds.append(m)  # noqa: E702
    m = z(); m[H - 1, W - 1] = 1; kinds.append(m)  # noqa: E702
    out = []
    for i in range(n):
        if n >= len(kinds) and i < len(kinds):
            out.append(kinds[i])
        elif n < len(kinds) and i == 0:
            out.append(kinds[4])
        else:
            out.append((rng.random((H, W)) < rng.choice([0.03, 0.5, 0.9])).astype(np.uint8))
    return out
