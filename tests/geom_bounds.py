"""Float64 references and element-wise error bounds for the stage-2/3 geometry ("glue") kernels of csrc/pp_geom.hip — similarity
volume, calc_pred_Ms, pose_recovery_2d, the initial and the stage-3 correspondences, the PnP gather — and for pp_simvol_backward.
A helper of tests/test_geom_bounds_{cpu,gpu}.py, imported through sys.path like tests/kernel_bounds.py; it needs nothing but torch.

    inputs(op, case)                 the seeded fp32 inputs of one case of the sweep CASES[op] (the shapes travel in the dict)
    reference(op, inp) -> (ref, bound)   float64 (exact operations: the exact integers / fp32 bits and what may differ)
    impl(op, inp, dtype, wrong=None)     the kernel's formula restated in torch in `dtype`: float32 = the independent fp32
                                         implementation that sets the margins; float64 + wrong = a structurally wrong variant
    ratio(op, got, ref, bound)       worst |got - ref| / bound; an exact operation gives 0 (equal) or inf

ref comes from torch's own float64 ops (F.normalize, einsum, F.interpolate(mode="nearest"), torch.linalg.inv, torch.sigmoid, plain
indexing), never from impl(), from oracle/ or from this project's kernels.  bound = MARGIN[op] x model, u = 2^-24, cs(n) =
log2(n) + 2 (the pairwise-summation figure of kernel_bounds).  The models:

* simvol  out[b, s, h, w] = relu(<q_hat_t, x_hat_s> m_s), t = w 16 + h, m the nearest 16 x 16 resample of the template mask.
  The kernel accumulates the raw dot product d = sum_c q_c x_c on the fp32 MFMA chain (C fma terms: cs(C) u sum|q_c x_c|) and the
  two sums of squares beside it; a norm is a sum of C positive terms (cs(C) u relative), a square root (halves it, rounds once)
  and one reciprocal / division: (cs(C)/2 + 2) u relative each; d rq, that times (m / |x|): with the mask's division three
  products, 3 u.  With A = sum_c |q_c x_c| / (|q| |x|) and S = <q_hat, x_hat>:
      model = u |m| (cs(C) A + (cs(C) + 7) |S|).
  ReLU is 1-Lipschitz.  Where the sampled mask is 0 the model is 0: the output must be exactly 0; a column of zeros (norm 0,
  clamped at 1e-12) gives A = S = 0: exactly 0 as well.  The nearest index min(floor(dst in/16), in - 1) has no rounding of its
  own: in/16 is exact in fp32 for every size and so is its product with dst <= 15.
* simvol_bwd  dS[b, t, s] = dout[b, s, h, w] m_s [out > 0]: one product per element, the same product torch's fp32 makes:
  bit-equal (margin 0) to torch.where(out > 0, dout * m, 0) on the same `out`; +0 and -0 are both "not > 0".
* pred_ms, pose2d: closed forms of a few dozen operations on 3 x 3 matrices, where a flat k u |y| is wrong in both directions
  (pixel-scale entries cancel in K^-1 and in t - A c).  Running-error bound: the kernel's expression tree is evaluated in float64
  on (value, error) pairs —
      a + b: e_a + e_b + u (|a| + |b|)      a b: |a| e_b + |b| e_a + u |a b|      a / b: (e_a + |a / b| e_b) / |b| + u |a / b|
      sqrt a: e_a / (2 sqrt a) + u sqrt a    constants (0, 1) and copies exact
  i.e. every product and sum is replaced by the sum of the absolute values of its terms times u times the roundings on the path,
  and the divisions by c[2], sc, det (through 1 / det) and z carry their operand's relative error.  Roundings on the longest path
  per output entry — pred_ms: [0][0..1], [1][0..1] one product: 1; [i][2]: K t 3 (product, two adds), / c[2] 1 (+ c[2]'s own 3),
  tem_M c 3, the 2 x 2 part 1, its product with the centre and the sum 2, trans 14 and its sum 2, the last difference 1: 16;
  last row constants: 0.  pose2d: R[i][j], i < 2: sc 3 (product, add, sqrt), the division 1, the row product 3: 7; R[2][j] copies:
  0; translation: c 7, inv 1, (inv pm) tM 6, aff c 3, K^-1 (2 x 2 minors 2, det 4 more, 1 / det 1, product 1: 8), K^-1 qc 3,
  / z 1 (+ z's own 14), qz (scale2d 3 on aff's 7, division, focal, product: 13) and the last product 1: about 40 on the path, which is why the
  bound is evaluated and not stated as a constant; last row copies: 0.
* init_corr  flow = (M p)_xy / (M p)_w / patch m - grid, certainty = m, p = the patch centre (w patch + patch/2, h patch +
  patch/2, 1), exact in fp32.  A numerator row is two products and two adds, 3 roundings on the path of sum_j |M_ij p_j|; the
  division by ww 1; by patch 1: 5.  ww's own error (3 u sum_j |M_2j p_j| / |ww| relative: the sweep's projective rows have
  M_2j >= 0, so that sum IS ww and never cancels — "ww kept away from 0"), the mask product and the last difference (one
  rounding each, u |f m| and u (|f m| + |grid|)) are of the size of the counted terms, and with fma contraction the kernel makes fewer
  of them; the measured margin covers them:
      model = u (5 sum_j |M_ij p_j| / |ww| / patch |m| + |grid|);      certainty bit-equal to the nearest sample (model 0).
* stage3  tar = trunc(flow + grid) where kept, else -1; src = (w, h) where kept; entry k = w H + h.  flow + grid is ONE fp32
  rounding in the reference as well, so the coordinates are compared exactly against the fp32 sum truncated toward zero, and so
  are the four inequalities (the reference's quirk x < H - 1, y < W - 1 included).  Only sigmoid(c) > thr involves a
  transcendental: sg = 1 / (1 + expf(-c)): expf at 1 ulp (ROCm ocml: exp 1 ulp for fp32) = 2 u of a value that, after the
  reciprocal, is scaled to <= 1; the add 1 u; the reciprocal 1 u: 4 u of a value <= 1.  With margin 2: a position is EXEMPT where
  |sigmoid_float64(c) - thr| <= 8 u = 2^-21 (thr as the fp32 number the kernel is handed); there either decision is accepted,
  everywhere else the decision is exact.  c = 0 is never exempt: expf(-0) = 1, 1 + 1 and 1 / 2 are exact, sg = 0.5 with no error,
  and 0.5 > 0.5 is false.  c = +-inf gives exactly 1 / 0.  Cap: at most 0.1 % of a case's positions may be exempt (random
  certainties of unit scale fall into a band of 2^-20 with probability ~1e-6) and none of the planted ones.
* gather  rows feat[b, :, y, x] of the entries with x != -1 and y != -1, order kept; count per item: no arithmetic, bit-equal to
  torch indexing.

Margins.  MARGIN[op] = at most 4 x the worst |err| / model of impl(op, ., float32) over the sweep, measured on the CPU by
tests/test_geom_bounds_cpu.py (which prints it), never from the HIP kernels: the _set(op, measured, margin) calls below and the
table in DESIGN.md.  Bit-equal operations (simvol_bwd, stage3, gather) have margin 0.

Dense query_K.  Real intrinsics are upper triangular: six of the nine adjugate entries are then multiplied by zeros and a wrong
index among them is invisible.  The "dense" family is K = K_real Rot(axis, 0.15 .. 0.35 rad): all nine entries non-zero,
det K = fx fy (|det| >= 2e5), cond_2 K = cond_2 K_real ~ 1e3 (a rotation changes neither), and the depth component of K^-1 qc
stays above 0.5.
"""
import math

import torch
import torch.nn.functional as F

import kernel_bounds as kb

U = 2.0 ** -24
cs = kb.cs
WORST = {}
MEASURED = {}
MARGIN = {}
BAND = 8 * U           # stage3: |sigmoid64(c) - thr| within it -> either decision
EXEMPT_CAP = 1e-3      # ... on at most this share of a case's positions


def _set(op, measured, margin):
    assert margin <= 4.0 * measured + 1e-12, (op, measured, margin)
    MEASURED[op], MARGIN[op] = measured, margin


_set("simvol", 0.73, 2.3)
_set("simvol_bwd", 0.0, 0.0)
_set("pred_ms", 0.981, 3.1)
_set("pose2d", 0.4, 1.3)
_set("init_corr", 0.716, 2.3)
_set("stage3", 0.0, 0.0)
_set("gather", 0.0, 0.0)
EXACT = ("simvol_bwd", "stage3", "gather")

# ------------------------------------------------------------------------------------------------------------------ the sweep
MASKS = [(224, 224), (16, 16), (37, 53), (100, 60), (17, 500)]
STAGE3_HW = [(64, 64), (8, 24), (24, 8), (5, 7), (1, 1), (16, 17)]
GATHER_N = [1, 63, 64, 65, 1023, 1024, 1025, 2500, 4096]
GATHER_KINDS = ["random", "last_chunk", "first_chunk"]

CASES = {
    "simvol": [dict(C=C, B=[1, 3][(i + j) % 2], mh=hw[0], mw=hw[1]) for i, C in enumerate([16, 48, 384, 1024]) for j, hw in enumerate(MASKS)],
    "simvol_bwd": [dict(B=B, mh=hw[0], mw=hw[1]) for B in [1, 2, 32, 33, 40] for hw in [(224, 224), (37, 53)]],
    "pred_ms": [dict(B=B) for B in [1, 63, 64, 65, 130]],
    "pose2d": [dict(B=B, K=fam) for B in [1, 63, 64, 65, 130] for fam in ("real", "dense")],
    "init_corr": [dict(size=s, B=B, projective=p) for s in [16, 32, 224, 448] for B in [1, 5] for p in (False, True)],
    "stage3": [dict(H=hw[0], W=hw[1], B=[1, 3][(i + j) % 2], thr=thr) for i, hw in enumerate(STAGE3_HW) for j, thr in enumerate([0.3, 0.5, 0.7])],
    "gather": [dict(N=N, C=[1, 3, 5][(i + r) % 3], H=[(64, 64), (5, 9)][(i + r) % 2][0], W=[(64, 64), (5, 9)][(i + r) % 2][1],
                    kind=GATHER_KINDS[(i + 2 * r) % 3]) for r in (0, 1) for i, N in enumerate(GATHER_N)],
}
OPS = list(CASES)


def case_name(op, c):
    return op + "(" + ",".join(f"{k}={v}" for k, v in c.items()) + ")"


def _gen(op, c, seed):
    return torch.Generator().manual_seed(7919 * OPS.index(op) + 31 * CASES[op].index(c) + seed if c in CASES[op] else 5 + seed)


def _mask(g, B, mh, mw):
    """non-binary: 0, 0.5, 1, 2 in blobs of a few pixels and single pixels (the kernels multiply by the value)"""
    vals = torch.tensor([0.0, 0.5, 1.0, 2.0])
    coarse = vals[torch.randint(0, 4, (B, -(-mh // 3), -(-mw // 3)), generator=g)]
    m = coarse.repeat_interleave(3, 1).repeat_interleave(3, 2)[:, :mh, :mw].clone()
    flip = torch.rand(B, mh, mw, generator=g) < 0.2
    return torch.where(flip, vals[torch.randint(0, 4, (B, mh, mw), generator=g)], m).contiguous()


def _rot(ax, ay, az):
    """Rz Ry Rx of (B,) angles, float64"""
    def m(rows):
        return torch.stack([torch.stack(r, -1) for r in rows], -2)
    o, z = torch.ones_like(ax), torch.zeros_like(ax)
    rx = m([[o, z, z], [z, ax.cos(), -ax.sin()], [z, ax.sin(), ax.cos()]])
    ry = m([[ay.cos(), z, ay.sin()], [z, o, z], [-ay.sin(), z, ay.cos()]])
    rz = m([[az.cos(), -az.sin(), z], [az.sin(), az.cos(), z], [z, z, o]])
    return rz @ ry @ rx


def _intrinsics(g, B):
    u = lambda lo, hi: torch.rand(B, generator=g, dtype=torch.float64) * (hi - lo) + lo   # noqa: E731
    K = torch.zeros(B, 3, 3, dtype=torch.float64)
    K[:, 0, 0], K[:, 1, 1] = u(520, 680), u(450, 515)               # fx != fy
    K[:, 0, 2], K[:, 1, 2] = u(250, 400), u(180, 300)               # off-centre principal point
    K[:, 0, 1] = u(-0.5, 0.5)
    K[:, 2, 2] = 1
    return K


def pose_inputs(B, fam, seed=0):
    """the inputs of pp_calc_pred_Ms and pp_pose_recovery_2d for B items: in-plane angles in all four quadrants, scales 0.25 .. 4,
    translations in [-1, 1], template depth 0.3 .. 3, tem_M a general crop affine (anisotropic, a little shear), query_M a valid
    crop affine, query_K real intrinsics or the dense family; pred_Ms = the float64 closed form rounded to fp32"""
    g = torch.Generator().manual_seed(4001 + 17 * B + (0 if fam == "real" else 1) + seed)
    u = lambda lo, hi: torch.rand(B, generator=g, dtype=torch.float64) * (hi - lo) + lo   # noqa: E731
    th = (torch.arange(B) % 4).double() * (math.pi / 2) + u(0.1, math.pi / 2 - 0.1)
    z = 0.3 * 10.0 ** u(0.0, 1.0)
    pose = torch.zeros(B, 4, 4, dtype=torch.float64)
    pose[:, :3, :3] = _rot(u(-3, 3), u(-1.4, 1.4), u(-3, 3))
    pose[:, 0, 3], pose[:, 1, 3], pose[:, 2, 3] = u(-0.2, 0.2) * z, u(-0.2, 0.2) * z, z
    pose[:, 3, 3] = 1
    tem_M = torch.zeros(B, 3, 3, dtype=torch.float64)
    tem_M[:, 0, 0], tem_M[:, 1, 1] = u(0.3, 2.0), u(0.3, 2.0)
    tem_M[:, 0, 1], tem_M[:, 1, 0] = u(-0.15, 0.15), u(-0.15, 0.15)
    tem_M[:, 0, 2], tem_M[:, 1, 2] = u(-100, 100), u(-100, 100)
    tem_M[:, 2, 2] = 1
    qM = torch.zeros(B, 3, 3, dtype=torch.float64)
    qM[:, 0, 0] = u(0.3, 2.0)
    qM[:, 1, 1] = qM[:, 0, 0]
    qM[:, 0, 2], qM[:, 1, 2] = u(-100, 100), u(-100, 100)
    qM[:, 2, 2] = 1
    qK = _intrinsics(g, B)
    if fam == "dense":
        axis = F.normalize(torch.randn(B, 3, generator=g, dtype=torch.float64) + torch.tensor([0.6, 0.6, 0.6]).double(), dim=1)
        ang = u(0.15, 0.35)
        kx = torch.zeros(B, 3, 3, dtype=torch.float64)
        kx[:, 0, 1], kx[:, 0, 2], kx[:, 1, 0], kx[:, 1, 2], kx[:, 2, 0], kx[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
        rot = torch.eye(3).double() + ang.sin().view(B, 1, 1) * kx + (1 - ang.cos()).view(B, 1, 1) * (kx @ kx)
        qK = qK @ rot
    d = dict(scale=0.25 * 16.0 ** u(0.0, 1.0), inplane=torch.stack([th.cos(), th.sin()], 1), trans=torch.stack([u(-1, 1), u(-1, 1)], 1),
             tem_pose=pose, tem_K=_intrinsics(g, B), tem_M=tem_M, query_M=qM, query_K=qK)
    d = {k: v.float() for k, v in d.items()}
    d["pred_Ms"] = _pred_ms_ref({k: v.double() for k, v in d.items()}, 14.0).float()
    d["trans_scale"] = 14.0
    return d


def _stage3_plants(H, W, thr):
    """(tx, ty, c) of the planted positions: all representable so that flow = target - grid and flow + grid are exact"""
    e = 2.0 ** -12
    inf, nan = float("inf"), float("nan")
    ix, iy = min(1.25, (H - 1) / 2), min(1.75, (W - 1) / 2)        # a point inside
    return [(ix, iy, 0.0), (ix, iy, inf), (ix, iy, -inf), (0.0, iy, 5.0), (H - 1.0, iy, 5.0), (e, iy, 5.0), (H - 1.0 - e, iy, 5.0),
            (ix, W - 1.0, 5.0), (ix, W - 1.0 - e, 5.0), (0.75, iy, 5.0), (nan, iy, 5.0), (ix, nan, 5.0), (ix, iy, nan), (ix, e, 5.0), (ix, 0.0, 5.0)]


def inputs(op, c, seed=0):
    g = _gen(op, c, seed)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    if op == "simvol":
        B, C = c["B"], c["C"]

        def feats():
            mag = 10.0 ** (torch.rand(1, C, 1, 1, generator=g) * 3 - 1.5)            # channel magnitudes over three decades
            x = rn(B, C, 16, 16) * mag
            return torch.sign(x + (x == 0)) * x.abs().clamp(1e-3, 1e3)
        src, tar = feats(), feats()
        src[0, :, 3, 5] = 0.0                                                           # columns of exact zeros: norm 0, the 1e-12 clamp
        tar[B - 1, :, 9, 2] = 0.0
        return dict(src=src, tar=tar, mask=_mask(g, B, c["mh"], c["mw"]))
    if op == "simvol_bwd":
        B = c["B"]
        r = torch.rand(B, 256, 16, 16, generator=g)
        out = rn(B, 256, 16, 16).abs()
        out = torch.where(r < 0.2, torch.zeros(()), torch.where(r < 0.4, -torch.zeros(()), torch.where(r < 0.5, torch.full((), 1e-30), out)))
        dout = rn(B, 256, 16, 16) * 10.0 ** (torch.rand(B, 256, 1, 1, generator=g) * 4 - 2)
        return dict(out=out, dout=dout, mask=_mask(g, B, c["mh"], c["mw"]))
    if op in ("pred_ms", "pose2d"):
        return pose_inputs(c["B"], c.get("K", "real"), seed)
    if op == "init_corr":
        B, size = c["B"], c["size"]
        u = lambda lo, hi: torch.rand(B, generator=g) * (hi - lo) + lo   # noqa: E731
        th, s = u(-math.pi, math.pi), 0.5 * 4.0 ** u(0.0, 1.0)
        M = torch.zeros(B, 3, 3)
        M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1] = s * th.cos(), -s * th.sin() * 1.1, s * th.sin(), s * th.cos() * 0.9
        M[:, 0, 2], M[:, 1, 2] = u(-0.4, 0.4) * size, u(-0.4, 0.4) * size
        M[:, 2, 2] = 1
        if c["projective"]:
            M[:, 2, 0], M[:, 2, 1] = u(0.05, 0.5) / size, u(0.05, 0.5) / size      # ww in [1, 2]: away from 0, no cancellation
        return dict(pred_Ms=M, mask=_mask(g, B, size, size))
    if op == "stage3":
        B, H, W, thr = c["B"], c["H"], c["W"], c["thr"]
        ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
        side = float(max(H, W))
        tx = torch.rand(B, H, W, generator=g) * (side + 1) - 1                        # targets over both sides' range and a little outside
        ty = torch.rand(B, H, W, generator=g) * (side + 1) - 1
        flow = torch.stack([tx - xs, ty - ys], 1)
        cert = rn(B, 1, H, W) * 2
        planted = []
        plants = _stage3_plants(H, W, thr)
        if H * W >= 2 * len(plants):
            step = (H * W) // len(plants)
            for i, (px, py, pc) in enumerate(plants):
                k = i * step + (i % step)
                h, w = k // W, k % W
                flow[0, 0, h, w], flow[0, 1, h, w], cert[0, 0, h, w] = px - w, py - h, pc
                planted.append((0, h, w))
        return dict(flow=flow, cert=cert, thr=thr, planted=planted)
    if op == "gather":
        N, C, H, W, kind = c["N"], c["C"], c["H"], c["W"], c["kind"]
        feat = rn(3, C, H, W)
        idx = torch.stack([torch.randint(0, W, (3, N), generator=g), torch.randint(0, H, (3, N), generator=g)], -1)
        n = torch.arange(N)
        # item 0: nothing valid — both -1, only x = -1, only y = -1 in turn
        idx[0, n % 3 != 1, 0] = -1
        idx[0, n % 3 != 2, 1] = -1
        # item 1: everything valid, positions in descending order with repeats
        p = torch.sort(torch.randint(0, H * W, (N,), generator=g), descending=True).values
        idx[1, :, 0], idx[1, :, 1] = p % W, p // W
        # item 2: mixed — invalid entries of all three kinds among valid ones; or valid entries in the first / the last chunk of 1024 only
        r = torch.rand(N, generator=g)
        last0 = ((N - 1) // 1024) * 1024
        dead = {"random": r < 0.45, "last_chunk": (n < last0) | (r < 0.3), "first_chunk": (n >= 1024) | (r < 0.3)}[kind]
        which = torch.randint(0, 3, (N,), generator=g)
        idx[2, dead & (which != 1), 0] = -1
        idx[2, dead & (which != 2), 1] = -1
        return dict(feat=feat, idx=idx)
    raise ValueError(op)


# ------------------------------------------------------------------------------------------- pieces shared by impl and the models
def _nearest_index(n_in, dt=torch.float32):
    i = torch.floor(torch.arange(16, dtype=dt) * (torch.tensor(float(n_in), dtype=dt) / 16)).long()
    return i.clamp_max(n_in - 1)


def _nearest16(mask):
    """the kernels' index rule, spelled out (impl only; the references use F.interpolate)"""
    return mask[:, _nearest_index(mask.shape[1])][:, :, _nearest_index(mask.shape[2])]


def _nearest16_ref(mask):
    return F.interpolate(mask[:, None].double(), size=(16, 16), mode="nearest")[:, 0]


def _to_out_layout(v_bts):
    """[b, t, s] with t = w 16 + h  ->  [b, s, h, w]"""
    B = v_bts.shape[0]
    return v_bts.permute(0, 2, 1).reshape(B, 256, 16, 16).permute(0, 1, 3, 2)


def _from_out_layout(o):
    """[b, s, h, w] -> [b, t, s], t = w 16 + h"""
    B = o.shape[0]
    return o.permute(0, 1, 3, 2).reshape(B, 256, 256).permute(0, 2, 1)


class E:
    """a float64 value with a first-order bound of its fp32 evaluation error (the running-error rules of the module docstring)"""

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def _w(o):
        return o if isinstance(o, E) else E(torch.as_tensor(o, dtype=torch.float64))

    def __add__(self, o):
        o = E._w(o)
        return E(self.v + o.v, self.e + o.e + U * (self.v.abs() + o.v.abs()))

    def __sub__(self, o):
        o = E._w(o)
        return E(self.v - o.v, self.e + o.e + U * (self.v.abs() + o.v.abs()))

    def __mul__(self, o):
        o = E._w(o)
        v = self.v * o.v
        return E(v, self.v.abs() * o.e + o.v.abs() * self.e + U * v.abs())

    def __truediv__(self, o):
        o = E._w(o)
        v = self.v / o.v
        return E(v, (self.e + v.abs() * o.e) / o.v.abs() + U * v.abs())

    def __neg__(self):
        return E(-self.v, self.e)

    def sqrt(self):
        r = self.v.sqrt()
        return E(r, self.e / (2 * r) + U * r)


def _sqrt(x):
    return x.sqrt()


def _mul3(a, b):
    return [a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j] for i in range(3) for j in range(3)]


def _mulv3(a, v):
    return [a[i * 3] * v[0] + a[i * 3 + 1] * v[1] + a[i * 3 + 2] * v[2] for i in range(3)]


def _entries(t, wrap):
    """(B, r, c) -> the list of r c (B,) entries, row-major"""
    return [wrap(t[:, i, j]) for i in range(t.shape[1]) for j in range(t.shape[2])]


def _pred_ms_tree(d, wrap, wrong=None):
    """pred_ms_kernel's expression tree on (B,) entries: tensors of any dtype, or E"""
    P, K, M = _entries(d["tem_pose"], wrap), _entries(d["tem_K"], wrap), _entries(d["tem_M"], wrap)
    t = [P[12], P[13], P[14]] if wrong == "translation_row" else [P[3], P[7], P[11]]
    c = _mulv3(K, t)
    c = [c[0] / c[2], c[1] / c[2], c[2] / c[2]]
    cm = _mulv3(M, c)
    s, co, si = wrap(d["scale"]), wrap(d["inplane"][:, 0]), wrap(d["inplane"][:, 1])
    m00, m01, m10, m11 = co * s, -si * s, si * s, co * s
    if wrong == "rotation_transposed":
        m01, m10 = m10, m01
    ax, ay = m00 * cm[0] + m01 * cm[1], m10 * cm[0] + m11 * cm[1]
    ts = d["trans_scale"]
    tx, ty = cm[0] + wrap(d["trans"][:, 0]) * ts, cm[1] + wrap(d["trans"][:, 1]) * ts
    zero, one = wrap(torch.zeros_like(d["scale"])), wrap(torch.ones_like(d["scale"]))
    return [m00, m01, tx - ax, m10, m11, ty - ay, zero, zero, one]


def _pose2d_tree(d, wrap, wrong=None):
    """pose2d_kernel's expression tree"""
    P, pm, qM = _entries(d["tem_pose"], wrap), _entries(d["pred_Ms"], wrap), _entries(d["query_M"], wrap)
    k, tK, tM = _entries(d["query_K"], wrap), _entries(d["tem_K"], wrap), _entries(d["tem_M"], wrap)
    zero, one = wrap(torch.zeros_like(d["pred_Ms"][:, 0, 0])), wrap(torch.ones_like(d["pred_Ms"][:, 0, 0]))
    sc = _sqrt(pm[0] * pm[0] + pm[3] * pm[3])
    rin = [pm[0] / sc, pm[1] / sc, zero, pm[3] / sc, pm[4] / sc, zero, zero, zero, one]
    rt = [P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]]
    R = _mul3(rt, rin) if wrong == "template_first" else _mul3(rin, rt)
    t = [P[12], P[13], P[14]] if wrong == "translation_row" else [P[3], P[7], P[11]]
    c = _mulv3(tK, t)
    c = [c[0] / c[2], c[1] / c[2], one]                  # (c[2] / c[2] is exactly 1)
    s = qM[0]
    inv = [one / s, zero, -qM[2] / s, zero, one / s, -qM[5] / s, zero, zero, one]
    aff = _mul3(_mul3(inv, pm), tM)
    qc = _mulv3(aff, c)
    det = k[0] * (k[4] * k[8] - k[5] * k[7]) - k[1] * (k[3] * k[8] - k[5] * k[6]) + k[2] * (k[3] * k[7] - k[4] * k[6])
    idet = one / det
    ik = [(k[4] * k[8] - k[5] * k[7]) * idet, (k[2] * k[7] - k[1] * k[8]) * idet, (k[1] * k[5] - k[2] * k[4]) * idet,
          (k[5] * k[6] - k[3] * k[8]) * idet, (k[0] * k[8] - k[2] * k[6]) * idet, (k[2] * k[3] - k[0] * k[5]) * idet,
          (k[3] * k[7] - k[4] * k[6]) * idet, (k[1] * k[6] - k[0] * k[7]) * idet, (k[0] * k[4] - k[1] * k[3]) * idet]
    if wrong == "adjugate_transposed":
        ik = [ik[0], ik[3], ik[6], ik[1], ik[4], ik[7], ik[2], ik[5], ik[8]]
    scale2d = _sqrt(aff[0] * aff[0] + aff[1] * aff[1]) if wrong == "scale_from_row" else _sqrt(aff[0] * aff[0] + aff[3] * aff[3])
    focal = one if wrong == "no_focal_ratio" else k[0] / tK[0]
    qz = (t[2] / scale2d) * focal
    qt = _mulv3(ik, qc)
    z = qt[2]
    return [R[0], R[1], R[2], (qt[0] / z) * qz, R[3], R[4], R[5], (qt[1] / z) * qz, R[6], R[7], R[8], (qt[2] / z) * qz, P[12], P[13], P[14], P[15]]


def _pred_ms_ref(d, trans_scale):
    """float64 closed form in matrix notation"""
    B = d["scale"].shape[0]
    c = torch.einsum("bij,bj->bi", d["tem_K"], d["tem_pose"][:, :3, 3])
    c = c / c[:, 2:3]
    cm = torch.einsum("bij,bj->bi", d["tem_M"], c)[:, :2]
    co, si = d["inplane"][:, 0], d["inplane"][:, 1]
    A = torch.stack([co, -si, si, co], 1).view(B, 2, 2) * d["scale"].view(B, 1, 1)
    out = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)
    out[:, :2, :2] = A
    out[:, :2, 2] = cm + d["trans"] * trans_scale - torch.einsum("bij,bj->bi", A, cm)
    return out


def _pose2d_ref(d):
    B = d["pred_Ms"].shape[0]
    pm, P = d["pred_Ms"], d["tem_pose"]
    rin = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)
    rin[:, :2, :2] = pm[:, :2, :2] / torch.linalg.vector_norm(pm[:, :2, 0], dim=1).view(B, 1, 1)
    out = P.clone()
    out[:, :3, :3] = rin @ P[:, :3, :3]
    c = torch.einsum("bij,bj->bi", d["tem_K"], P[:, :3, 3])
    c = c / c[:, 2:3]
    qM = d["query_M"]
    inv = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)           # the crop affine's inverse (isotropic scale + translation)
    inv[:, 0, 0] = inv[:, 1, 1] = 1 / qM[:, 0, 0]
    inv[:, :2, 2] = -qM[:, :2, 2] / qM[:, 0, 0:1]
    aff = inv @ pm @ d["tem_M"]
    qc = torch.einsum("bij,bj->bi", aff, c)
    qt = torch.einsum("bij,bj->bi", torch.linalg.inv(d["query_K"]), qc)
    qz = P[:, 2, 3] / torch.linalg.vector_norm(aff[:, :2, 0], dim=1) * (d["query_K"][:, 0, 0] / d["tem_K"][:, 0, 0])
    out[:, :3, 3] = qt / qt[:, 2:3] * qz.view(B, 1)
    return out


def _stage3_layout(t_bhwc):
    """"b h w c -> b (w h) c": entry k = w H + h"""
    B, H, W, C = t_bhwc.shape
    return t_bhwc.permute(0, 2, 1, 3).reshape(B, H * W, C)


# ------------------------------------------------------------------------------------------------------------- the formulas in torch
def impl(op, inp, dtype=torch.float32, wrong=None):
    """The operation as the kernel is specified to compute it, in `dtype`; wrong: the name of a structural error (WRONG[op])."""
    t = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}
    if op == "simvol":
        src, tar = t["src"], t["tar"]
        B, C = src.shape[:2]
        x, q = src.reshape(B, C, 256), tar.reshape(B, C, 256)
        nx, nq = (x * x).sum(1), (q * q).sum(1)
        if wrong != "squared_norm":
            nx, nq = torch.sqrt(nx), torch.sqrt(nq)
        nx, nq = nx.clamp_min(1e-12), nq.clamp_min(1e-12)
        m16 = _nearest16(t["mask"])
        if wrong == "mask_xy_swapped":          # mask[nearest(sx), nearest(sy)]
            m16 = m16.transpose(1, 2)
        m = m16.reshape(B, 256)
        S = torch.einsum("bct,bcs->bts", q, x)
        if wrong == "mask_on_query":
            v = S * (m / nq)[:, :, None] * (1.0 / nx)[:, None, :]
        else:
            v = S * (1.0 / nq)[:, :, None] * (m / nx)[:, None, :]
        v = F.relu(v)
        if wrong == "t_hw":                     # t = h 16 + w
            return v.permute(0, 2, 1).reshape(B, 256, 16, 16)
        return _to_out_layout(v)
    if op == "simvol_bwd":
        out, dout = t["out"], t["dout"]
        B = out.shape[0]
        m = _nearest16(t["mask"]).reshape(B, 256, 1, 1)
        if wrong == "mask_by_t":
            m = _nearest16(t["mask"]).transpose(1, 2).reshape(B, 1, 16, 16).expand(B, 256, 16, 16)    # the mask of patch t = w 16 + h
        d = torch.where(out >= 0 if wrong == "ge" else out > 0, dout * m, torch.zeros((), dtype=dtype))
        if wrong == "t_hw":
            return d.reshape(B, 256, 256).permute(0, 2, 1)
        return _from_out_layout(d)
    if op == "pred_ms":
        return torch.stack(_pred_ms_tree(t, lambda v: v, wrong), 1).view(-1, 3, 3)
    if op == "pose2d":
        return torch.stack(_pose2d_tree(t, lambda v: v, wrong), 1).view(-1, 4, 4)
    if op == "init_corr":
        M, mask = t["pred_Ms"], t["mask"]
        B, size = mask.shape[0], mask.shape[1]
        patch = float(size // 16)
        m = _nearest16(mask)
        i = torch.arange(16, dtype=dtype)
        cen = i * patch + (0.0 if wrong == "no_half_patch" else patch * 0.5)
        px, py = cen.view(1, 1, 16).expand(B, 16, 16), cen.view(1, 16, 1).expand(B, 16, 16)       # [b][h][w]: x from w, y from h
        if wrong == "k_hw":
            px, py = py, px
        e = lambda r, c: M[:, r, c].view(B, 1, 1)   # noqa: E731
        x = e(0, 0) * px + e(0, 1) * py + e(0, 2)
        y = e(1, 0) * px + e(1, 1) * py + e(1, 2)
        ww = e(2, 0) * px + e(2, 1) * py + e(2, 2)
        fx, fy = (x / ww) / patch, (y / ww) / patch
        gx, gy = i.view(1, 1, 16), i.view(1, 16, 1)
        if wrong == "mask_after_grid":
            flow = torch.stack([(fx - gx) * m, (fy - gy) * m], 1)
        else:
            flow = torch.stack([fx * m - gx, fy * m - gy], 1)
        return flow, m.view(B, 1, 16, 16)
    if op == "stage3":
        flow, cert, thr = inp["flow"], inp["cert"], inp["thr"]          # the coordinate sum is fp32 by specification
        B, _, H, W = flow.shape
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        tx, ty = flow[:, 0] + xs.float(), flow[:, 1] + ys.float()
        c = cert[:, 0].to(dtype)
        sg = 1.0 / (1.0 + torch.exp(-c))
        thr_t = torch.tensor(thr, dtype=torch.float32).to(dtype)
        hx, hy = (W - 1, H - 1) if wrong == "bounds_swapped" else (H - 1, W - 1)
        keep = (sg >= thr_t if wrong == "ge" else sg > thr_t) & (tx > 0) & (ty > 0) & (tx < hx) & (ty < hy)
        txy = torch.stack([tx, ty], -1)
        txy = torch.where(keep[..., None], txy, torch.zeros(()))
        tv = torch.round(txy).long() if wrong == "rounded" else txy.long()
        neg = torch.full((), -1, dtype=torch.long)
        tar = torch.where(keep[..., None], tv, neg)
        src = torch.where(keep[..., None], torch.stack([xs, ys], -1).expand(B, H, W, 2), neg)
        if wrong == "k_hw":
            return tar.reshape(B, H * W, 2), src.reshape(B, H * W, 2)
        return _stage3_layout(tar), _stage3_layout(src)
    if op == "gather":
        feat, idx = t["feat"], inp["idx"]
        B, C, H, W = feat.shape
        N = idx.shape[1]
        counts, rows = [], []
        for b in range(B):
            out = torch.full((N, C), float("nan"), dtype=dtype)
            base = 0
            for n0 in range(0, N, 1024):                                  # the kernel's chunks of 1024 entries with the carried base
                x, y = idx[b, n0:n0 + 1024, 0], idx[b, n0:n0 + 1024, 1]
                v = (x != -1) & (y != -1)
                p = (x * H + y if wrong == "index_xH_y" else y * W + x)[v]
                cnt = int(v.sum())
                at = 0 if wrong == "base_dropped" else base
                out[at:at + cnt] = feat[b].reshape(C, H * W)[:, p % (H * W)].t()
                base += cnt
            counts.append(base)
            rows.append(out[:base])
        return torch.tensor(counts, dtype=torch.int32), rows
    raise ValueError(op)


# -------------------------------------------------------------------------------------------------------------- references and models
def model(op, inp):
    """(ref, model): torch's float64 result and the un-margined error model; exact operations: (exact result, what may differ)"""
    d = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}
    if op == "simvol":
        B, C = d["src"].shape[:2]
        x, q = d["src"].reshape(B, C, 256), d["tar"].reshape(B, C, 256)
        xh, qh = F.normalize(x, dim=1), F.normalize(q, dim=1)
        S = torch.einsum("bct,bcs->bts", qh, xh)
        A = torch.einsum("bct,bcs->bts", qh.abs(), xh.abs())
        m = _nearest16_ref(d["mask"]).reshape(B, 1, 256)
        k = cs(C)
        return _to_out_layout(F.relu(S * m)), _to_out_layout(U * m.abs() * (k * A + (k + 7) * S.abs()))
    if op == "simvol_bwd":
        out, dout = inp["out"], inp["dout"]                                # fp32 on purpose: the one product is torch's own fp32 product
        B = out.shape[0]
        m = _nearest16_ref(inp["mask"]).float().reshape(B, 256, 1, 1)
        return _from_out_layout(torch.where(out > 0, dout * m, torch.zeros(()))).contiguous(), None
    if op == "pred_ms":
        tree = _pred_ms_tree(d, E)
        return _pred_ms_ref(d, d["trans_scale"]), torch.stack([t.e for t in tree], 1).view(-1, 3, 3)
    if op == "pose2d":
        tree = _pose2d_tree(d, E)
        return _pose2d_ref(d), torch.stack([t.e for t in tree], 1).view(-1, 4, 4)
    if op == "init_corr":
        M, mask = d["pred_Ms"], d["mask"]
        B, size = mask.shape[0], mask.shape[1]
        patch = size // 16
        m = _nearest16_ref(mask)
        cen = torch.arange(16, dtype=torch.float64) * patch + patch / 2
        yy, xx = torch.meshgrid(cen, cen, indexing="ij")                   # [h][w]
        p = torch.stack([xx, yy, torch.ones_like(xx)], -1)
        moved = torch.einsum("bij,hwj->bhwi", M, p)
        absum = torch.einsum("bij,hwj->bhwi", M.abs(), p.abs())
        ww = moved[..., 2:3]
        gy, gx = torch.meshgrid(torch.arange(16.0, dtype=torch.float64), torch.arange(16.0, dtype=torch.float64), indexing="ij")
        grid = torch.stack([gx, gy], 0)[None]
        flow = (moved[..., :2] / ww / patch).permute(0, 3, 1, 2) * m[:, None] - grid
        mod = U * (5 * (absum[..., :2] / ww.abs() / patch).permute(0, 3, 1, 2) * m[:, None].abs() + grid)
        return (flow, m[:, None]), (mod, torch.zeros_like(m[:, None]))
    if op == "stage3":
        flow, cert = inp["flow"], inp["cert"]
        B, _, H, W = flow.shape
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        tx, ty = flow[:, 0] + xs.float(), flow[:, 1] + ys.float()          # ONE fp32 rounding, in the reference as in the kernel
        inside = (tx > 0) & (ty > 0) & (tx < H - 1) & (ty < W - 1)
        sig = torch.sigmoid(cert[:, 0].double())
        thr = float(torch.tensor(inp["thr"], dtype=torch.float32))
        keep = (sig > thr) & inside
        exempt = ((sig - thr).abs() <= BAND) & (cert[:, 0] != 0) & inside
        txy = torch.where(inside[..., None], torch.stack([tx, ty], -1), torch.zeros(()))
        kept_tar, kept_src = torch.trunc(txy).long(), torch.stack([xs, ys], -1).expand(B, H, W, 2)
        neg = torch.full((), -1, dtype=torch.long)
        ref = (_stage3_layout(torch.where(keep[..., None], kept_tar, neg)), _stage3_layout(torch.where(keep[..., None], kept_src, neg)))
        return ref, dict(exempt=_stage3_layout(exempt[..., None])[..., 0], kept_tar=_stage3_layout(kept_tar), kept_src=_stage3_layout(kept_src),
                         exempt_bhw=exempt)
    if op == "gather":
        feat, idx = inp["feat"], inp["idx"]
        counts, rows = [], []
        for b in range(feat.shape[0]):
            x, y = idx[b, :, 0], idx[b, :, 1]
            v = (x != -1) & (y != -1)
            rows.append(feat[b][:, y[v], x[v]].t().contiguous())           # plain indexing feat[b, :, y, x]
            counts.append(int(v.sum()))
        return (torch.tensor(counts, dtype=torch.int32), rows), None
    raise ValueError(op)


def reference(op, inp):
    """(ref, bound) = (torch's float64 result, MARGIN[op] x model)"""
    ref, m = model(op, inp)
    if op in EXACT:
        return ref, m
    k = MARGIN[op]
    return ref, (tuple(k * t for t in m) if isinstance(m, tuple) else k * m)


def ratio(op, got, ref, bound):
    """worst |got - ref| / bound (0 / 0 = 0, a NaN = inf); exact operations: 0.0 where everything agrees, inf otherwise"""
    if op == "simvol_bwd":
        g = got.detach().cpu()
        return 0.0 if g.shape == ref.shape and g.dtype == ref.dtype and torch.equal(g, ref) else float("inf")
    if op == "stage3":
        tar, src = got[0].cpu(), got[1].cpu()
        if tar.shape != ref[0].shape or tar.dtype != torch.int64 or src.dtype != torch.int64:
            return float("inf")
        same = (tar == ref[0]).all(-1) & (src == ref[1]).all(-1)
        kept = (tar == bound["kept_tar"]).all(-1) & (src == bound["kept_src"]).all(-1)
        dropped = (tar == -1).all(-1) & (src == -1).all(-1)
        ok = same | (bound["exempt"] & (kept | dropped))
        return 0.0 if bool(ok.all()) else float("inf")
    if op == "gather":
        counts, rows = got
        if not torch.equal(counts.cpu().to(torch.int32), ref[0]):
            return float("inf")
        return 0.0 if all(a.shape == b.shape and torch.equal(a.cpu(), b) for a, b in zip(rows, ref[1])) else float("inf")
    if not isinstance(ref, tuple):
        got, ref, bound = (got,), (ref,), (bound,)
    w = 0.0
    for a, r, b in zip(got, ref, bound):
        a = a.detach().cpu().double()
        if a.shape != r.shape:
            return float("inf")
        err = (a - r).abs()
        q = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))      # (a NaN is not == 0: NaN / b = NaN)
        q = torch.nan_to_num(q, nan=float("inf"), posinf=float("inf"))
        if q.numel():
            w = max(w, float(q.max()))
    return w


def check(op, name, got, ref, bound):
    """assert the kernel's result against (ref, bound) of reference(); prints and records the worst |err| / bound"""
    r = ratio(op, got, ref, bound)
    finite = True
    if op not in EXACT:
        finite = all(bool(torch.isfinite(g).all()) for g in (got if isinstance(got, tuple) else (got,)))
    print(f"[bound] {name}: worst |err|/bound = {r:.3g}" + (" (exact)" if op in EXACT else ""), flush=True)
    if r > WORST.get(op, (-1.0, ""))[0]:
        WORST[op] = (r, name)
    assert finite, f"{name}: non-finite output"
    assert r <= 1.0, f"{name}: |err| / bound = {r:.3g}"
    return r


# wrong implementation -> the rule under which a case contains its error
WRONG = {
    "simvol": {"t_hw": lambda c: True, "mask_xy_swapped": lambda c: True, "mask_on_query": lambda c: True, "squared_norm": lambda c: True},
    "simvol_bwd": {"t_hw": lambda c: True, "mask_by_t": lambda c: True, "ge": lambda c: True},
    "pred_ms": {"translation_row": lambda c: True, "rotation_transposed": lambda c: True},
    "pose2d": {"template_first": lambda c: True, "no_focal_ratio": lambda c: True, "scale_from_row": lambda c: True,
               "adjugate_transposed": lambda c: True, "translation_row": lambda c: True},
    "init_corr": {"k_hw": lambda c: True, "no_half_patch": lambda c: True, "mask_after_grid": lambda c: True},
    # (1 x 1 has one entry and nothing inside; >= differs from > only at the planted c = 0 against thr = 0.5)
    "stage3": {"k_hw": lambda c: c["H"] * c["W"] > 1, "bounds_swapped": lambda c: c["H"] != c["W"], "rounded": lambda c: c["H"] * c["W"] > 1,
               "ge": lambda c: c["thr"] == 0.5 and c["H"] * c["W"] > 1},
    "gather": {"index_xH_y": lambda c: c["N"] >= 63, "base_dropped": lambda c: c["N"] > 1024},
}
