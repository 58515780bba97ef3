"""Float64 references and element-wise error bounds for the fused self-attention (csrc/pp_attn.hip: attn_kernel, attn_f16x3_kernel in its
register-staged, ring and resident variants) and its recomputing adjoint (csrc/pp_attn_bwd.hip).  A helper of
tests/test_attn_bounds_{cpu,gpu}.py, imported through sys.path like tests/corr_bounds.py; it reuses engine_bounds (TAU, FLOOR_ACT, check, WORST)
and kernel_bounds (U, cs, the activation-split term of an operand output).

    inputs(op, case)                              fp32 CPU tensors: qkv (B T, 3 heads 64), and dout (B T, heads 64) for the adjoint
    reference(op, case, inp, mode) -> (ref, bound)  float64 CPU tensors in the kernels' layouts (a tuple dq, dk, dv for the adjoint)
    impl(op, case, inp, dtype, mode, wrong=None)  the kernels' formula restated in torch in `dtype`: float32 sets the margins, float64 + wrong is
                                                  a structurally wrong variant with the quantisers kept

Ops: attn (the output, (B T, heads 64)), attn_lse (the base-2 log-sum-exp of the scaled scores the training forward keeps, (B heads, T)),
attn_bwd (dq, dk, dv, each (B T, heads 64): the three column blocks of dqkv).  head_dim is 64 and scale = 1 / 8 everywhere.

ref comes from torch's own float64 ops only: p = softmax(q k^T / 8), out = p v per image and head, lse = logsumexp(q k^T / 8) / ln 2, the adjoint
float64 autograd of exactly that forward with the given dout.  Never oracle/, impl() or this project's kernels.

impl restates the kernels.  Keys go in chunks of 32 with the online maximum m and sum l in the base-2 domain; T % 32 <= 4 keys are folded in one
at a time after the chunks (exact fp32 products of the operands' values, the probability not split), otherwise the last chunk is partial; the
accumulators are rescaled by alpha = exp2(m_old - m_new) (the kernel skips the multiplication when alpha == 1 for a whole wave: the same
values).  f32 (attn_kernel): q is prescaled by fl(scale log2 e), p = exp2(s - m), out = o (1 / l).  Operand modes (attn_f16x3_kernel): q, k, v as
hi = f16(4 x), lo = f16(4 x - hi); raw scores hi hi + hi lo + lo hi (f16x3) or hi hi (f16); the maximum on the raw sums, x = exp2(fma(raw,
fl(scale log2 e) / 16, 10 - m)) = 1024 p, split the same way (no factor 4), l summed from the unsplit x in those units; out = o (0.25 / l);
lse = m + log2(l) - 10.  MFMA accumulation order is approximated by a torch product in `dtype`, the fma by one rounding of the double result.
The adjoint (f16x3 only): g = 2^k with max|dout| g in [512, 1024) (autograd._pow2_scale), D = g sum_d dO O from the forward's fp32 O, raw
scores as above, p = exp2(raw S_DESCALE - lse) with the forward's lse, dP = (3-term product of split(g dO) and split(v)) / 16,
dS = p (dP - D); every 32 x 32 tile of dS is split with its own power of two per column (a query in the dq kernel, a key in the dk kernel)
so that the column maximum lands in [512, 1024) (biased exponent clamped to [40, 250]); P for dV is min(p, 2) 1024 in two terms;
dq = dS K scale / (4 g), dk = dS^T Q scale / (4 g), dv = P^T (g dO) / (4 g 1024).

Models, u = 2^-24, per image, head and query i, A_ij = sum_d |q_id| |k_jd| / 8, s = q k^T / 8 (natural units), m = max_j s_ij, p = softmax(s).
First-order perturbation of the soft-max: |dp_j| <= p_j (|ds_j| + sum_i p_i |ds_i|).
* ds_ij, the error of the exponential's argument:
    f32:      (cs(64) + 2) u A + u (2 |s| + |s - m|)            the 64-term fma chain, the prescale of q by a rounded constant; s rounds, s - m rounds
    operand:  TAU64[mode] A + FLOOR_ACT (sum_d |q_id| + sum_d |k_jd|) / 8 + u (2 |s| + |s - m| + 7)
              engine_bounds' contraction model re-derived for 64 terms (TAU64 below: eb.TAU is sized for K up to 16 384); S_DESCALE is a rounded constant and m = fl(max S_DESCALE): 2 u |s|; the fma's one rounding of
              s2 - m2 + 10 (10 ln 2 = 7 in natural units)
* attn:  rel_ij = ds_ij + sum_k p_ik ds_ik + (cs(T) + 6) u   (v_exp_f32 1 ulp = 2 u, the sum of T positive terms with its rescales, the
  reciprocal and the final product), dp = p rel, in the operand modes + r p + 2^-35 max_j p_ij: the split of 1024 p (r = 2^-22, 2^-11 in f16) and
  its subnormal grid: 2^-25 in x = 2^-35 in the probability relative to the running maximum, which the later rescales and the
  normalisation by l >= 1 / max p only shrink — a probability below it is dropped, the reference's is not;
      model = sum_j dp_ij |v_jd| + sum_j p_ij (r |v_jd| + FLOOR_ACT) [operand] + cs(T) u sum_j p_ij |v_jd| + 2 u |out|
  Operand output: + kernel_bounds' activation-split term of the result (2^-22 |out| + 2^-27, 2^-11 |out| + 2^-27 for one term).
* attn_lse (base 2; invariant to the stored maximum: l is summed against the same m):
      model = log2 e (sum_j p_ij ds_ij + (cs(T) + 6) u) + u (3 log2(1024 l) + |m2| + 2 |lse| + 10)       v_log_f32 1 ulp, the two additions
* attn_bwd, with P recomputed: rp_ij = ds_ij(f16x3, without the 7) + ln 2 m_lse_i + u (3 + |ln p_ij|), dP = dO V^T,
      ddP = TAU64 sum_d |dO_id| |v_jd| + FLOOR_ACT (sum_d |dO_id| + sum_d |v_jd| / g)       the g-scaled floor of split(g dO): 2^-27 / g per element
      dD_i = sum_d |dO_id| m_out_id + (cs(64) + 2) u sum_d |dO_id O_id|                     the error of the forward's O inside D
      ddS  = p rp |dP - D| + p (ddP + dD) + 2 u |dS| + 2^-22 |dS| + 2^-35 colmax_tile + 2^-121
  colmax_tile = the largest |dS| of the element's column within its 32-row tile: over the 32 keys of a chunk for a query (dq), over the 32
  queries of a chunk for a key (dk) — the term a single global scale would blow up to 2^-35 max |dS|.
      m_dq = (ddS_q |K| + |dS| (2^-22 |K| + FLOOR_ACT) + cs(T) u |dS| |K|) / 8 + 2 u |dq|         and the same with dS^T, Q for dk
      m_dv = (p rp + 2^-22 p + 2^-35)^T |dO| + p^T (2^-22 |dO| + FLOOR_ACT / g) + cs(T) u p^T |dO| + 2 u |dv|
No exemptions: the soft-max has no kink, every element of every output is held to its bound.

Margins: MARGIN[key] <= 4 x the worst |impl - ref| / model over the sweep, measured on the CPU by tests/test_attn_bounds_cpu.py from
impl(float32) in the mode's arithmetic (the emulated splits for f16x3 / f16), never from the HIP kernels; set at about 3 x the measured value.
One margin per mode for attn, one for attn_lse, one each for dq, dk, dv.
The unfused chain (batched GEMMs and the soft-max row kernels: the f32 engine's route, and the f16x3 engine's with FUSED_ATTENTION off) is held to
the same references and the fused bounds, with one exception: its f16x3 adjoint splits dS with ONE power of two for the whole tensor and the
kept P at scale 4, so dk and dv of a key that receives little attention carry the floor 2^-27 / g2 of every dS element resp. 2^-27 of every
probability — the terms the per-tile ranging and the 1024 p operand of the fused kernels remove.  That adjoint gets the model terms
(2 x 2^-27 / g2) sum_j |K_jd| / 8 (dq), the same with Q (dk), 2^-27 sum_i |dO_id| (dv), and margins of its own (unfused_f16x3:*), measured from
the chain's restatement in torch float32 with the emulated splits; its forward stays on the fused bound, and the fused bounds are not widened.
"""
import math

import torch

import engine_bounds as eb
import kernel_bounds as kb

U = kb.U
cs = kb.cs
check = eb.check
worst_ratio = kb.worst_ratio
MEASURED, MARGIN = {}, {}
HD, KC, TAILMAX = 64, 32, 4
SCALE = HD ** -0.5
LOG2E = 1.44269504088896340736
LN2 = math.log(2.0)
MODES = ("f32", "f16x3", "f16")
R_SPLIT = {"f16x3": 2.0 ** -22, "f16": 2.0 ** -11}
P_FLOOR = 2.0 ** -35
# the contraction model of engine_bounds for the 64 terms of a head: eb.TAU is sized for K up to 16 384 (2^-18 = 8 x the operand error); over 64
# terms its own derivation gives the operand errors and the dropped lo lo product, 2^-21, plus the fp32 accumulation cs(64) u; f16: the two
# 11-bit roundings 2^-10 on top; f32: the fma chain and the prescale of q
TAU64 = {"f32": (cs(HD) + 2) * U, "f16x3": 2.0 ** -21 + cs(HD) * U, "f16": 2.0 ** -10 + 2.0 ** -21 + cs(HD) * U}


def _set(op, measured, margin):
    assert margin <= 4.0 * measured + 1e-12, (op, measured, margin)
    MEASURED[op], MARGIN[op] = measured, margin


_set("attn:f32", 0.393, 1.2)
_set("attn:f16x3", 0.503, 1.5)
_set("attn:f16", 0.37, 1.1)
_set("attn_lse", 0.425, 1.3)
_set("attn_bwd:dq", 0.0605, 0.18)
_set("attn_bwd:dk", 0.0901, 0.27)
_set("attn_bwd:dv", 0.28, 0.84)
# the adjoint of the unfused chain in f16x3 (FUSED_ATTENTION off): its own model terms (one global scale for dS, P split at scale 4), measured
# from the restatement of that chain with the emulated splits; its forward is held to the fused bound
_set("unfused_f16x3:dq", 0.0418, 0.125)
_set("unfused_f16x3:dk", 0.0587, 0.176)
_set("unfused_f16x3:dv", 0.144, 0.43)

KINDS = ("normal", "peaked", "flat", "first_key", "last_key", "big_v", "heads_decades", "small", "near_range")
DOUTS = ("unit", "rows_decades", "tiny", "large")
# T -> the path it is the smallest size of (the table of DESIGN.md)
TS = (1, 3, 4, 5, 31, 32, 33, 36, 37, 64, 96, 100, 129, 161, 257, 260, 261, 289)


def _cases():
    small_bh = [(1, 1), (1, 3), (4, 2), (3, 3)]           # B heads = 1, 3, 8, 9: idle ids of the XCD-interleaved grid, an exact round, a second round
    big_bh = [(1, 1), (1, 3), (3, 1), (1, 2)]
    fwd = []
    for i, T in enumerate(TS):
        B, heads = (small_bh if T <= 129 else big_bh)[i % 4]
        fwd.append(dict(B=B, T=T, heads=heads, kind="normal"))
    for j, kind in enumerate(KINDS[1:]):
        Tsmall = (3, 4)[j % 2]
        fwd.append(dict(B=(1, 3)[j % 2], T=Tsmall, heads=3, kind=kind))
        fwd.append(dict(B=(3, 4, 1)[j % 3], T=37, heads=(3, 2, 3)[j % 3], kind=kind))
        fwd.append(dict(B=1, T=257, heads=(3, 2)[j % 2], kind=kind))
    fwd.append(dict(B=1, T=260, heads=2, kind="last_key"))
    fwd.append(dict(B=1, T=261, heads=2, kind="first_key"))
    fwd.append(dict(B=2, T=33, heads=1, kind="flat"))
    bwd = []
    for i, (T, B, heads, kind, dout) in enumerate([
            (1, 1, 2, "normal", "unit"), (3, 1, 3, "normal", "rows_decades"), (4, 3, 1, "peaked", "unit"), (5, 1, 1, "normal", "tiny"),
            (31, 1, 3, "flat", "large"), (32, 4, 2, "normal", "unit"), (33, 2, 1, "normal", "rows_decades"), (33, 3, 3, "flat", "unit"),
            (37, 3, 3, "normal", "rows_decades"), (37, 1, 3, "peaked", "unit"), (37, 1, 3, "heads_decades", "unit"), (37, 4, 2, "first_key", "tiny"),
            (37, 1, 1, "last_key", "large"), (37, 1, 3, "small", "rows_decades"), (64, 2, 3, "peaked", "large"), (100, 1, 3, "normal", "tiny"),
            (129, 3, 3, "normal", "unit"), (161, 1, 1, "peaked", "rows_decades"), (257, 1, 3, "normal", "rows_decades"), (257, 1, 2, "peaked", "unit"),
            (257, 1, 2, "last_key", "unit"), (260, 1, 2, "heads_decades", "large"), (289, 1, 1, "normal", "unit")]):
        bwd.append(dict(B=B, T=T, heads=heads, kind=kind, dout=dout))
    return dict(attn=fwd, attn_lse=fwd, attn_bwd=bwd)


CASES = _cases()
OPS = list(CASES)
# the four cases of the unfused chain (batched GEMMs + the soft-max row kernels)
UNFUSED = [c for c in CASES["attn_bwd"] if (c["T"], c["kind"]) in ((3, "normal"), (37, "normal"), (64, "peaked"), (257, "normal"))]


def case_name(op, c):
    return op + "(" + ",".join(f"{k}={v}" for k, v in c.items()) + ")"


def case_id(c):
    return "-".join(str(v) for v in c.values())


# ------------------------------------------------------------------------------------------------------------------ inputs
def _split_heads(x, c):
    """(B T, n heads 64) -> n tensors (B, heads, T, 64)"""
    B, T, H = c["B"], c["T"], c["heads"]
    return x.view(B, T, -1, H, HD).permute(2, 0, 3, 1, 4)


def _rows(t):
    """(B, heads, T, 64) -> (B T, heads 64)"""
    B, H, T, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * T, H * HD)


def inputs(op, c, seed=0):
    B, T, H, kind = c["B"], c["T"], c["heads"], c["kind"]
    g = kb._gen(11000 + seed + 131 * T + 17 * B + 5 * H + 7 * KINDS.index(kind) + 1000 * DOUTS.index(c.get("dout", "unit")))
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    q, k, v = rn(B, H, T, HD), rn(B, H, T, HD), rn(B, H, T, HD)
    w = (torch.randint(0, 2, (B, H, 1, HD), generator=g) * 2 - 1).float()          # a sign direction of norm 8 per image and head
    if kind == "peaked":
        q, k = q * 4, k * 4
    elif kind == "flat":
        q, k = q * 0.05, k * 0.05
    elif kind in ("first_key", "last_key"):
        # the planted key scores 1.3^2 64 / 8 = 13.5 natural units above the others (whose scores have std 0.7) for every query
        j = 0 if kind == "first_key" else T - 1
        q, k = 0.5 * q + 1.3 * w, 0.5 * k
        k[:, :, j] += 1.3 * w[:, :, 0]
    elif kind == "big_v":
        # key j: score -1.5^2 64 / 8 = -18 for every query (p < 1e-6 already at T = 3), its v row 8000
        j = T // 2
        q = q + 1.5 * w
        k[:, :, j] = -1.5 * w[:, :, 0] + 0.25 * k[:, :, j]
        v[:, :, j] = 8000.0
    elif kind == "heads_decades":
        hs = torch.arange(H, dtype=torch.float32).view(1, H, 1, 1)
        q, k, v = q * 0.5 ** hs, k * 0.5 ** hs, v * 10.0 ** -hs
    elif kind == "small":
        lim = 2.0 ** -5 * 0.99
        q, k, v = ((t * 2.0 ** -7).clamp(-lim, lim) for t in (q, k, v))
    elif kind == "near_range":
        # a few elements at 1.5e4 (the operand format saturates at 16 376), q and k in different dimensions: scores of a few thousand
        for t, d in ((q, 3), (k, 7), (v, 11)):
            n = max(1, T // 16)
            idx = torch.randperm(T, generator=g)[:n]
            t[:, :, idx, d] = 1.5e4 * (torch.randint(0, 2, (B, H, n), generator=g) * 2 - 1).float()
    qkv = torch.cat([_rows(q), _rows(k), _rows(v)], 1).contiguous()
    d = dict(qkv=qkv)
    if op == "attn_bwd":
        do = rn(B * T, H * HD)
        dk_ = c["dout"]
        if dk_ == "rows_decades":
            do[::3] *= 1e-3
        elif dk_ == "tiny":
            do *= 1e-7
        elif dk_ == "large":
            do *= 30.0
        d["dout"] = do
    return d


# ------------------------------------------------------------------------------------------------------------------ the float64 reference
def ref_forward(qkv, c):
    """(out (B T, heads 64), lse2 (B heads, T), p (B, heads, T, T)) in qkv's dtype, differentiable"""
    q, k, v = _split_heads(qkv, c)
    s = q @ k.transpose(-1, -2) * SCALE
    p = torch.softmax(s, -1)
    return _rows(p @ v), (torch.logsumexp(s, -1) / LN2).reshape(c["B"] * c["heads"], c["T"]), p


def ref_backward(qkv, dout, c):
    x = qkv.double().clone().requires_grad_(True)
    ref_forward(x, c)[0].backward(dout.double())
    C = c["heads"] * HD
    return x.grad[:, :C], x.grad[:, C:2 * C], x.grad[:, 2 * C:]


# ------------------------------------------------------------------------------------------------------ the kernels' formula in torch
def _q16(a):
    """a (fp32-exact values) rounded to fp16 with the kernels' clamp, in a's dtype"""
    return a.float().clamp(-65504.0, 65504.0).half().to(a.dtype)


def _split(x, terms, mul=4.0):
    """the operand terms of x as values at the operand's scale: hi = f16(mul x), lo = f16(mul x - hi) (None for one term)"""
    a = (x.float() * mul).to(x.dtype)
    hi = _q16(a)
    return hi, (_q16(a - hi) if terms == 2 else None)


def _prod(a, b, drop=None):
    """a b^T over the last axis of the split operands a = (hi, lo), b = (hi, lo): hi hi + hi lo + lo hi, or hi hi alone"""
    (ah, al), (bh, bl) = a, b
    out = ah @ bh.transpose(-1, -2)
    if al is not None:
        out = out + ah @ bl.transpose(-1, -2)
        if drop != "lo_hi":
            out = out + al @ bh.transpose(-1, -2)
    return out


def _consts(dtype, wrong=None):
    l2e = float(torch.tensor(LOG2E).half()) if wrong == "log2e_11bits" else LOG2E
    sc2 = float(torch.tensor(l2e, dtype=torch.float32)) * SCALE if dtype == torch.float32 else l2e * SCALE      # (scale = 2^-3: exact)
    return sc2, sc2 / 16.0


def _fma(a, b, c_):
    """a b + c with one rounding"""
    return (a.double() * b + c_.double()).to(a.dtype)


def _forward(q, k, v, mode, wrong=None):
    """(out, lse2) as (B, heads, T, 64) and (B, heads, T) in q's dtype"""
    dt = q.dtype
    B, H, T, _ = q.shape
    ntail = T % KC if T % KC <= TAILMAX else 0
    Tm = T - ntail
    sc2, sdesc = _consts(dt, wrong)
    o = torch.zeros(B, H, T, HD, dtype=dt)
    mrun = torch.full((B, H, T), float("-inf"), dtype=dt)
    lrun = torch.zeros(B, H, T, dtype=dt)
    lse = None
    op_mode = mode != "f32"
    terms = 2 if mode == "f16x3" else 1
    if op_mode:
        qs, ks, vs = _split(q, terms), _split(k, terms), _split(v, terms)
        cut = lambda t, a, b: (t[0][:, :, a:b], None if t[1] is None else t[1][:, :, a:b])   # noqa: E731
    else:
        qs = q * sc2
    for k0 in range(0, Tm, KC):
        k1 = min(k0 + KC, Tm)
        if op_mode:
            raw = _prod(qs, cut(ks, k0, k1), "lo_hi" if wrong == "lohi_dropped" else None)          # (queries x keys), units 16 q.k
        else:
            raw = qs @ k[:, :, k0:k1].transpose(-1, -2)
        if wrong == "masked_counted" and k1 - k0 < KC:                                              # the masked keys of a partial chunk: score 0
            raw = torch.cat([raw, torch.zeros(B, H, T, KC - (k1 - k0), dtype=dt)], -1)
        mx = raw.max(-1).values
        mnew = torch.maximum(mrun, mx * sdesc if op_mode else mx)
        alpha = torch.exp2(mrun - mnew)
        if op_mode:
            x = torch.exp2(_fma(raw, sdesc, (10.0 - mnew).unsqueeze(-1)))                             # 1024 p
        else:
            x = torch.exp2(raw - mnew.unsqueeze(-1))
        lrun = lrun * alpha + x.sum(-1)
        mrun = mnew
        x = x[..., :k1 - k0]
        if wrong != "no_rescale":
            o = o * alpha.unsqueeze(-1)
        if op_mode:
            ph = _q16(x.float().to(dt))
            pl = _q16(x.float().to(dt) - ph) if (terms == 2 and wrong != "p_lo_dropped") else None
            vh, vl = cut(vs, k0, k1)
            o = o + ph @ vh
            if vl is not None:
                o = o + ph @ vl
            if pl is not None:
                o = o + pl @ vh
        else:
            o = o + x @ v[:, :, k0:k1]
    if wrong == "lse_before_tail":
        lse = mrun + torch.log2(lrun) - (10.0 if op_mode else 0.0)
    for kx in (range(Tm, T) if wrong != "tail_dropped" else ()):
        if op_mode:
            qv = qs[0] + (qs[1] if qs[1] is not None else 0.0)
            kv = ks[0][:, :, kx] + (ks[1][:, :, kx] if ks[1] is not None else 0.0)
            vv = vs[0][:, :, kx] + (vs[1][:, :, kx] if vs[1] is not None else 0.0)
            sv = (qv * kv.unsqueeze(2)).sum(-1) * sdesc
        else:
            sv = (qs * k[:, :, kx].unsqueeze(2)).sum(-1)
            vv = v[:, :, kx]
        mnew = torch.maximum(mrun, sv)
        alpha = torch.exp2(mrun - mnew)
        pw = torch.exp2(sv - mnew + 10.0) if op_mode else torch.exp2(sv - mnew)
        lrun = lrun * alpha + pw
        mrun = mnew
        o = vv.unsqueeze(2) * pw.unsqueeze(-1) + (o if wrong == "no_rescale" else o * alpha.unsqueeze(-1))
    if lse is None:
        lse = mrun + torch.log2(lrun) - (10.0 if op_mode else 0.0)
    inv = (0.25 if op_mode else 1.0) / lrun
    return o * inv.unsqueeze(-1), lse


def pow2_scale(t):
    """autograd._pow2_scale: g = 2^k with max|t| g in [512, 1024)"""
    m = float(t.abs().max())
    if not (m > 0.0 and math.isfinite(m)):
        return 1.0
    return 2.0 ** max(-100, min(100, 10 - math.frexp(m)[1]))


def _ranged(x, dim, global_scale=False):
    """split_ranged: x (fp32 values in x's dtype) split in two fp16 terms with one power of two per column of each tile (the maximum over
    `dim`, kept), the maximum landing in [512, 1024); returns hi / sc, lo / sc"""
    x32 = x.float()
    mx = x32.abs().amax(tuple(range(x.dim())) if global_scale else dim, keepdim=True)
    e8 = (torch.frexp(mx)[1] + 126).clamp(40, 250)
    e8 = torch.where(mx > 0, e8, torch.full_like(e8, 40))
    sc = torch.ldexp(torch.ones_like(mx), 136 - e8).to(x.dtype)
    v = (x32.to(x.dtype) * sc).clamp(-65504.0, 65504.0)
    hi = _q16(v)
    lo = _q16(v - hi)
    return hi / sc, lo / sc


def _backward(q, k, v, do, out, lse, wrong=None):
    """(dq, dk, dv) as (B, heads, T, 64) in q's dtype: the f16x3 adjoint with the forward's out and lse"""
    dt = q.dtype
    B, H, T, _ = q.shape
    nt = -(-T // KC)
    Tp = nt * KC
    g = pow2_scale(do)
    _, sdesc = _consts(dt)
    idx = torch.arange(Tp).clamp_max(T - 1)
    inside = (torch.arange(Tp) < T).to(dt)
    o_used = out.half().to(dt) if wrong == "D_from_fp16_O" else out
    D = ((do * o_used).sum(-1) * g)[:, :, idx]
    qs, ks, vs = (_split(t[:, :, idx], 2) for t in (q, k, v))
    gs = _split(do[:, :, idx] * g, 2)
    if wrong == "do_lo_dropped":
        gs = (gs[0], torch.zeros_like(gs[0]))
    raw = _prod(qs, ks)                                                    # (queries x keys)
    pacc = _prod(gs, vs)
    p = torch.exp2(raw * sdesc - lse[:, :, idx].unsqueeze(-1))
    ds = p * (pacc * (1.0 / 16.0) - D.unsqueeze(-1))
    keys_in, queries_in = inside.view(1, 1, 1, Tp), inside.view(1, 1, Tp, 1)
    ds_q = ds if wrong == "dq_keys_past_T" else ds * keys_in
    ds_k = ds if wrong == "dkv_queries_past_T" else ds * queries_in
    p_v = p if wrong == "dkv_queries_past_T" else p * queries_in
    glob = wrong == "ds_global_scale"
    xh, xl = _ranged(ds_q.reshape(B, H, Tp, nt, KC), 4, glob)              # per query, per tile of 32 keys
    xh, xl = xh.reshape(B, H, Tp, Tp), xl.reshape(B, H, Tp, Tp)
    dq = (xh @ ks[0] + xh @ ks[1] + xl @ ks[0]) * (SCALE / g / 4.0)
    yh, yl = _ranged(ds_k.reshape(B, H, nt, KC, Tp), 3, glob)              # per key, per tile of 32 queries
    yh, yl = yh.reshape(B, H, Tp, Tp).transpose(-1, -2), yl.reshape(B, H, Tp, Tp).transpose(-1, -2)
    dk = (yh @ qs[0] + yh @ qs[1] + yl @ qs[0]) * (SCALE / g / 4.0)
    x = (p_v.clamp_max(2.0) * 1024.0).float().to(dt)
    ph = _q16(x)
    pl = _q16(x - ph)
    ph, pl = ph.transpose(-1, -2), pl.transpose(-1, -2)
    dv = (ph @ gs[0] + ph @ gs[1] + pl @ gs[0]) * (1.0 / (g * 4.0 * 1024.0))
    return dq[:, :, :T], dk[:, :, :T], dv[:, :, :T]


def _unfused(q, k, v, do=None, split=False):
    """the unfused chain restated in q's dtype: S = q k^T / 8, row soft-max, P v; the adjoint from the kept P.  split: the f16x3 engine's batched
    products (both operands split on the fly at scale 4, three terms), the gradients dO and dS range-normalised first with ONE power of two
    for the whole tensor (autograd._ranged) — the forward quantities q, k, v, P as they are"""
    t_ = lambda x: x.transpose(-1, -2)   # noqa: E731
    if split:
        mm = lambda a, b: _prod(_split(a, 2), _split(t_(b), 2)) * (1.0 / 16.0)   # noqa: E731
    else:
        mm = lambda a, b: a @ b   # noqa: E731
    s = mm(q, t_(k)) * SCALE
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)
    out = mm(p, v)
    if do is None:
        return out
    g = pow2_scale(do) if split else 1.0
    dp = mm(do * g, t_(v)) / g
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    g2 = pow2_scale(ds) if split else 1.0
    return out, (mm(ds * g2, k) * (SCALE / g2), mm(t_(ds) * g2, q) * (SCALE / g2), mm(t_(p), do * g) / g)


def impl(op, c, inp, dtype=torch.float32, mode="f32", wrong=None):
    """the kernels' formula restated in torch in `dtype`; mode: the arithmetic (the adjoint and the log-sum-exp exist in f16x3 alone, "unfused":
    the unfused chain); wrong: a structural error of WRONG[op]"""
    q, k, v = (t.to(dtype) for t in _split_heads(inp["qkv"], c))
    if mode in ("unfused", "unfused_f16x3"):
        if op == "attn":
            return _rows(_unfused(q, k, v, split=mode == "unfused_f16x3"))
        do = _split_heads(inp["dout"], c)[0].to(dtype)
        return tuple(_rows(t) for t in _unfused(q, k, v, do, split=mode == "unfused_f16x3")[1])
    if op == "attn":
        return _rows(_forward(q, k, v, mode, wrong)[0])
    if op == "attn_lse":
        return _forward(q, k, v, "f16x3", wrong)[1].reshape(c["B"] * c["heads"], c["T"])
    do = _split_heads(inp["dout"], c)[0].to(dtype)
    out, lse = _forward(q, k, v, "f16x3")
    if dtype == torch.float64:                                             # (the kernels hand both on as fp32)
        out, lse = out.float().double(), lse.float().double()
    return tuple(_rows(t) for t in _backward(q, k, v, do, out, lse, wrong))


# ------------------------------------------------------------------------------------------------------------------ the models
def _fwd_model(c, inp, mode):
    """float64 pieces of the forward model: dict with out, m_out, lse, m_lse (kernel layouts) and the per-head tensors the adjoint needs"""
    q, k, v = (t.double() for t in _split_heads(inp["qkv"], c))
    T = c["T"]
    s = q @ k.transpose(-1, -2) * SCALE
    m = s.max(-1, keepdim=True).values
    p = torch.softmax(s, -1)
    lse_n = torch.logsumexp(s, -1)
    A = q.abs() @ k.abs().transpose(-1, -2) * SCALE
    if mode == "f32":
        ds0 = TAU64[mode] * A
        arg = U * (2 * s.abs() + (s - m).abs())
    else:
        ds0 = TAU64[mode] * A + eb.FLOOR_ACT * SCALE * (q.abs().sum(-1, keepdim=True) + k.abs().sum(-1).unsqueeze(-2))
        arg = U * (2 * s.abs() + (s - m).abs() + 7.0)
    ds = ds0 + arg
    E = (p * ds).sum(-1, keepdim=True)
    dp = p * (ds + E + (cs(T) + 6) * U)
    av = v.abs()
    out = p @ v
    if mode != "f32":
        r = R_SPLIT[mode]
        dp = dp + r * p + P_FLOOR * p.max(-1, keepdim=True).values
        m_rest = p @ (r * av + eb.FLOOR_ACT)
    else:
        m_rest = 0.0
    m_rest = m_rest + cs(T) * U * (p @ av) + 2 * U * out.abs()
    m_out = dp @ av + m_rest
    lse2 = lse_n / LN2
    l1024 = (lse_n - m[..., 0]) / LN2 + 10.0                              # log2(1024 l)
    m_lse = LOG2E * (E[..., 0] + (cs(T) + 6) * U) + U * (3 * l1024.abs() + (m[..., 0] / LN2).abs() + 2 * lse2.abs() + 10.0)
    return dict(q=q, k=k, v=v, s=s, p=p, out=out, m_out=m_out, dp=dp, m_rest=m_rest, lse=lse2, m_lse=m_lse, ds=ds0 + U * (2 * s.abs() + (s - m).abs()))


def _tile_max(x, dim):
    """the largest |x| of every tile of 32 along `dim` (-1 or -2), broadcast back"""
    T = x.shape[dim]
    nt = -(-T // KC)
    pad = nt * KC - T
    a = x.abs()
    if dim == -1:
        a = torch.nn.functional.pad(a, (0, pad))
        mx = a.reshape(*a.shape[:-1], nt, KC).amax(-1, keepdim=True).expand(*a.shape[:-1], nt, KC).reshape(a.shape)
        return mx[..., :T]
    a = torch.nn.functional.pad(a, (0, 0, 0, pad))
    sh = a.shape
    mx = a.reshape(*sh[:-2], nt, KC, sh[-1]).amax(-2, keepdim=True).expand(*sh[:-2], nt, KC, sh[-1]).reshape(sh)
    return mx[..., :T, :]


def model(op, c, inp, mode="f32", unfused=False):
    """(ref, un-margined model) in the kernels' layouts (tuples for the adjoint); unfused: the adjoint model of the unfused chain in f16x3"""
    B, T, H = c["B"], c["T"], c["heads"]
    if op == "attn":
        f = _fwd_model(c, inp, mode)
        return _rows(f["out"]), _rows(f["m_out"])
    f = _fwd_model(c, inp, "f16x3")
    if op == "attn_lse":
        return f["lse"].reshape(B * H, T), f["m_lse"].reshape(B * H, T)
    q, k, v, p, s = f["q"], f["k"], f["v"], f["p"], f["s"]
    do = _split_heads(inp["dout"], c)[0].double()
    g = pow2_scale(inp["dout"])
    r, fl = 2.0 ** -22, eb.FLOOR_ACT
    lnp = s - torch.logsumexp(s, -1, keepdim=True)
    rp = f["ds"] + LN2 * f["m_lse"].unsqueeze(-1) + U * (3 + lnp.abs())
    dP = do @ v.transpose(-1, -2)
    ddP = TAU64["f16x3"] * (do.abs() @ v.abs().transpose(-1, -2)) + fl * (do.abs().sum(-1, keepdim=True) + v.abs().sum(-1).unsqueeze(-2) / g)
    D = (do * f["out"]).sum(-1, keepdim=True)
    dD = (f["dp"] * dP.abs()).sum(-1, keepdim=True) + (do.abs() * f["m_rest"]).sum(-1, keepdim=True) + (cs(HD) + 2) * U * (do * f["out"]).abs().sum(-1, keepdim=True)
    dS = p * (dP - D)
    ddS = p * rp * (dP - D).abs() + p * (ddP + dD) + (2 * U + r) * dS.abs() + 2.0 ** -121
    ddS_q = ddS + P_FLOOR * _tile_max(dS, -1)
    ddS_k = ddS + P_FLOOR * _tile_max(dS, -2)
    aS = dS.abs()
    dq, dk, dv = dS @ k * SCALE, dS.transpose(-1, -2) @ q * SCALE, p.transpose(-1, -2) @ do
    m_dq = SCALE * (ddS_q @ k.abs() + aS @ (r * k.abs() + fl) + cs(T) * U * (aS @ k.abs())) + 2 * U * dq.abs()
    m_dk = SCALE * (ddS_k.transpose(-1, -2) @ q.abs() + aS.transpose(-1, -2) @ (r * q.abs() + fl) + cs(T) * U * (aS.transpose(-1, -2) @ q.abs())) \
        + 2 * U * dk.abs()
    pt = p.transpose(-1, -2)
    m_dv = (p * rp + r * p + P_FLOOR).transpose(-1, -2) @ do.abs() + pt @ (r * do.abs() + fl / g) + cs(T) * U * (pt @ do.abs()) + 2 * U * dv.abs()
    if unfused:
        # dS is split with ONE power of two g2 for the whole tensor (max|dS| g2 in [512, 1024); a factor 2 for a maximum that rounds across a
        # power of two): the subnormal floor 2^-27 / g2 <= 2^-35 max|dS| per element of dS, over all T terms of a sum; P is kept in fp32 and
        # split at scale 4 like any activation: 2^-27 per probability, where the fused kernels split 1024 p (2^-35)
        fl2 = 2.0 * fl / pow2_scale(dS)
        m_dq = m_dq + SCALE * fl2 * k.abs().sum(-2, keepdim=True)
        m_dk = m_dk + SCALE * fl2 * q.abs().sum(-2, keepdim=True)
        m_dv = m_dv + fl * do.abs().sum(-2, keepdim=True)
    return ref_backward(inp["qkv"], inp["dout"], c), (_rows(m_dq), _rows(m_dk), _rows(m_dv))


BWD_KEYS = ("attn_bwd:dq", "attn_bwd:dk", "attn_bwd:dv")
UNFUSED_KEYS = ("unfused_f16x3:dq", "unfused_f16x3:dk", "unfused_f16x3:dv")


def reference(op, c, inp, mode="f32", out_terms=0, unfused=False):
    """(ref, bound) = (torch's float64 result, MARGIN x model); out_terms: 2 / 1 adds the operand-format split of the result; unfused: the
    adjoint of the unfused chain in f16x3, its own model terms and margins"""
    ref, m = model(op, c, inp, mode, unfused)
    if op == "attn":
        b = MARGIN["attn:" + mode] * m
        return ref, (b + kb._split_bound(ref, out_terms) if out_terms else b)
    if op == "attn_lse":
        return ref, MARGIN["attn_lse"] * m
    keys = UNFUSED_KEYS if unfused else BWD_KEYS
    return ref, tuple(MARGIN[key] * t for key, t in zip(keys, m))


def _ntail(c):
    return c["T"] % KC if c["T"] % KC <= TAILMAX else 0


# wrong variant -> (the rule it breaks, the rule under which a case can show it, the case at which it MUST leave the bound)
WRONG = {
    "attn": {
        "tail_dropped": ("the T % 32 <= 4 keys after the chunks are folded in", lambda c: _ntail(c) > 0, dict(T=257, kind="flat")),
        "masked_counted": ("the keys past T of a partial chunk take no part", lambda c: c["T"] % KC > TAILMAX, dict(T=37, kind="normal")),
        "no_rescale": ("the accumulators are rescaled when the maximum moves", lambda c: c["T"] > 1, dict(T=257, kind="last_key")),
        "p_lo_dropped": ("the probability operand has two terms in f16x3", lambda c: c["T"] > TAILMAX, dict(T=37, kind="flat")),
        "lohi_dropped": ("K Q^T is three products in f16x3", lambda c: True, dict(T=257, kind="peaked")),
        "log2e_11bits": ("log2 e is an fp32 constant", lambda c: c["T"] > 1, dict(T=257, kind="peaked")),
    },
    "attn_lse": {
        "lse_before_tail": ("the log-sum-exp counts the tail keys", lambda c: _ntail(c) > 0, dict(T=257, kind="flat")),
    },
    "attn_bwd": {
        "ds_global_scale": ("every dS tile has its own power of two per column", lambda c: c["T"] > 1, dict(T=257, kind="peaked")),
        "dq_keys_past_T": ("keys past T are zeroed in dq", lambda c: c["T"] % KC != 0, dict(T=37, kind="normal")),
        "dkv_queries_past_T": ("queries past T take no part in dk and dv", lambda c: c["T"] % KC != 0, dict(T=33, kind="normal")),
        "do_lo_dropped": ("g dO is split in two terms", lambda c: True, dict(T=257, dout="rows_decades")),
        "D_from_fp16_O": ("D is taken from the fp32 output", lambda c: True, dict(T=257, kind="normal")),
    },
}


def named(op, w):
    """the cases at which variant w of op must leave the bound"""
    want = WRONG[op][w][2]
    return [c for c in CASES[op] if all(c.get(k_) == v_ for k_, v_ in want.items())]
