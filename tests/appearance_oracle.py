"""Numpy float64 statement of the appearance score (TEST INFRASTRUCTURE, not collected): include/picopose_hip.h, THE APPEARANCE SCORE,
and picopose_amd/proposals.py restated from their definitions.  It imports nothing from the package (proposal_oracle only): the
patch-validity rule, the cosines with the masked maximum (lowest index among equals) and its margin to the runner-up, the masked
mean, the combined score, the pipeline of label_proposals(appearance=True) after the descriptors, the error bounds, and the seeded
inputs the CPU and GPU tests share.

Error bounds, from the kernel's stated orders and proposal_oracle's derivation (u = 2^-24, gamma(n) = n u / (1 - n u); the raw rows
are fp32 numbers and exact inputs of both sides).

1. A cosine.  Points 1-2 of proposal_oracle's docstring hold for ANY summation order of the C products, so they cover THE CHAIN
   ORDER (one fma per channel, k ascending: C roundings): the unit rows carry delta(C) = gamma(C) / 2 + 4 u each, the chain
   gamma(C), and  e_cos(C) = gamma(C) + 2 delta(C) = 2 gamma(C) + 8 u.
2. patch_sim is a maximum of cosines over a fixed set of template patches.  A maximum of values that are each perturbed by at most
   e_cos moves by at most e_cos (whichever patch wins on either side).
3. app = (sum of the n_valid selected patch_sim) / n_valid.  The sum in THE ROW ORDER is some order of n_valid terms:
   |fl(sum) - sum| <= gamma(n_valid) sum |s_i| <= gamma(n_valid) n_valid (1 + e_cos); divided by n_valid that is
   gamma(n_valid) (1 + e_cos) on the mean, on top of the e_cos the terms themselves carry; the division adds u relative, at most u
   (1 + e_cos) absolute.
4. Second-order terms (delta^2, gamma delta, u e_cos) are below 1e-3 of the total for C, N <= 1024: one factor 1.01.
       sim_bound(C)    = 1.01 e_cos(C)
       app_bound(C, n) = 1.01 (e_cos(C) + gamma(n) (1 + e_cos(C)) + u)
   Nothing in them was read off the kernel's output.  The float64 side's own error is nine orders below and not counted.

patch_arg is compared only where the float64 margin between the best and the second-best valid template patch exceeds 2 e_cos
(each side of the comparison may move by e_cos); `undecided` counts the (proposal, patch) cells that leaves out and the tests cap
their share.  Planted cases may leave nothing out."""
import numpy as np

import proposal_oracle as po

U, gamma = po.U, po.gamma


def e_cos(C):
    return 2.0 * gamma(C) + 8.0 * U


def sim_bound(C):
    return 1.01 * e_cos(C)


def app_bound(C, n):
    return 1.01 * (e_cos(C) + gamma(n) * (1.0 + e_cos(C)) + U)


def patch_valid(mask, p):
    """mask (n, S, S) -> (valid (n, N) uint8, n_valid (n,) int32): patch i = py * w0 + px is valid iff 2 * count >= p * p, count the
    pixels of its cell with mask > 0.5 (False for a NaN)."""
    mask = np.asarray(mask)
    n, S = mask.shape[:2]
    w0 = S // p
    with np.errstate(invalid="ignore"):
        on = (mask > np.float32(0.5)).astype(np.int64)
    count = on.reshape(n, w0, p, w0, p).sum(axis=(2, 4)).reshape(n, w0 * w0)
    valid = (2 * count >= p * p).astype(np.uint8)
    return valid, valid.sum(1).astype(np.int32)


def appearance(query, q_valid, bank, t_valid, pair_row, unit_bank=False):
    """Raw fp32 rows query (P, N, C), bank (R, N, C) -> dict(patch_sim (P, N), patch_arg (P, N), margin (P, N), n_valid (P,), app
    (P,)), float64.  unit_bank: the bank rows are taken as they are (the device's own unit rows)."""
    query, bank = np.asarray(query, np.float64), np.asarray(bank, np.float64)
    P, N, C = query.shape
    sim, arg, margin = np.zeros((P, N)), np.full((P, N), -1, np.int64), np.full((P, N), np.inf)
    n_valid, app = np.zeros(P, np.int32), np.zeros(P)
    for p in range(P):
        r = int(pair_row[p])
        tv = np.asarray(t_valid[r]) != 0
        qv = np.asarray(q_valid[p]) != 0
        n_valid[p] = qv.sum()
        if not tv.any():
            continue
        q = po.normalize(query[p])
        t = bank[r] if unit_bank else po.normalize(bank[r])
        cos = np.where(tv[None], q @ t.T, -np.inf)
        arg[p] = np.argmax(cos, axis=1)                          # numpy's argmax returns the first of equal maxima
        s = -np.sort(-cos, axis=1)
        sim[p] = s[:, 0]
        if tv.sum() > 1:
            margin[p] = s[:, 0] - s[:, 1]
        if qv.any():
            app[p] = sim[p][qv].sum() / qv.sum()
    return {"patch_sim": sim, "patch_arg": arg, "margin": margin, "n_valid": n_valid, "app": app}


def undecided(m, C):
    """-> the (proposal, patch) cells whose patch_arg the bound cannot decide."""
    return int((m["margin"] <= 2.0 * e_cos(C)).sum())


def combine(semantic, app, weight):
    return (np.asarray(semantic, np.float64) + float(weight) * np.asarray(app, np.float64)) / (1.0 + float(weight))


def label_pipeline(desc, bank_unit, offsets, obj_ids, segmentations, tokens, q_valid, patch_unit, patch_valid_bank, weight=1.0, topk=5,
                   min_score=0.5, max_detections=100, nms_iou=0.25):
    """label_proposals(appearance=True) after the descriptors: the semantic match, cut and cap of proposal_oracle.label_pipeline;
    the survivors in ascending proposal index; their appearance against bank row offsets[label] + view (the device's unit rows taken
    as they are); the combined score; NMS in descending combined score, the lower index first among equals.
    -> list of (proposal index, object id, score, view, semantic, appearance), best first."""
    m = po.match(desc, bank_unit, offsets, topk, unit_bank=True)
    order = sorted(range(len(desc)), key=lambda a: (-m["best"][a], a))
    cand = sorted([a for a in order if m["best"][a] > min_score][:max_detections])
    if not cand:
        return []
    label = m["label"][cand]
    view = m["view"][cand, label]
    a = appearance(np.asarray(tokens)[cand], np.asarray(q_valid)[cand], patch_unit, patch_valid_bank, np.asarray(offsets)[label] + view,
                   unit_bank=True)
    score = combine(m["best"][cand], a["app"], weight)
    segs = [segmentations[c] for c in cand]
    kept = po.nms(score, label, po.intersections(segs), po.pack_bits(segs)[1], nms_iou)
    return [(cand[k], obj_ids[int(label[k])], float(score[k]), int(view[k]), float(m["best"][cand[k]]), float(a["app"][k])) for k in kept]


# ---- seeded inputs shared by the CPU and GPU tests -------------------------------------------------------------------------------------
N_SET, C_SET, P_SET, R = (1, 16, 65, 256), (8, 384, 1024), (1, 3, 5), 4
PAIR_ROWS = {1: (2,), 3: (2, 0, 2), 5: (3, 1, 3, 0, 2)}        # not monotonic, one view used twice
PATTERNS = ("all", "half", "one", "no_query", "no_template")
# planted rows need room: 10 % noise puts the planted cosine at 0.995, which 128 other random rows in 8 dimensions can reach
PLANTED_N, PLANTED_C = (16, 65, 256), (384, 1024)
SEED = 0                # fixed: the float64 side alone stays inside the cap for every case (tests/test_appearance_cpu.py asserts it)
UNDECIDED_CAP = 0.10


def _half(rng, shape):
    v = (rng.random(shape) < 0.5).astype(np.uint8)
    v[..., 0] |= (v.sum(-1) == 0).astype(np.uint8)              # (never an empty row: the empty cases are patterns of their own)
    return v


def random_case(P, N, C, pattern, seed=SEED):
    """Gaussian rows -> (query (P, N, C), q_valid (P, N), bank (R, N, C), t_valid (R, N), pair_row (P,))."""
    rng = np.random.default_rng([seed, P, N, C, PATTERNS.index(pattern)])
    query = rng.standard_normal((P, N, C)).astype(np.float32)
    bank = rng.standard_normal((R, N, C)).astype(np.float32)
    q_valid, t_valid = np.ones((P, N), np.uint8), np.ones((R, N), np.uint8)
    if pattern != "all":
        q_valid, t_valid = _half(rng, (P, N)), _half(rng, (R, N))
    if pattern == "one":
        q_valid[:], t_valid[:] = 0, 0
        q_valid[np.arange(P), rng.integers(0, N, P)] = 1
        t_valid[np.arange(R), rng.integers(0, N, R)] = 1
    if pattern == "no_query":
        q_valid[:] = 0
    if pattern == "no_template":
        t_valid[:] = 0
    return query, q_valid, bank, t_valid, np.asarray(PAIR_ROWS[P], np.int32)


def planted_case(P, N, C, seed=SEED):
    """Every query patch i of proposal p = template patch perm[p][i] of view pair_row[p] + 10 % noise (0.1 N(0, 1) on rows of unit
    variance), perm drawn among the VALID template patches (half of them); half the query patches valid.
    -> (query, q_valid, bank, t_valid, pair_row, perm (P, N))."""
    rng = np.random.default_rng([seed, P, N, C, 99])
    bank = rng.standard_normal((R, N, C)).astype(np.float32)
    t_valid, q_valid = _half(rng, (R, N)), _half(rng, (P, N))
    pair_row = np.asarray(PAIR_ROWS[P], np.int32)
    perm = np.stack([rng.choice(np.nonzero(t_valid[r])[0], N) for r in pair_row])
    query = np.stack([bank[r][perm[p]] for p, r in enumerate(pair_row)]) + 0.1 * rng.standard_normal((P, N, C))
    return query.astype(np.float32), q_valid, bank, t_valid, pair_row, perm
