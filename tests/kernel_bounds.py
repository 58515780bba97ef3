"""Float64 references and element-wise error bounds for the kernels BETWEEN the contractions: bilinear resize, feature warp, 2 x 2
average pooling, LayerNorm, GroupNorm(+ReLU), BatchNorm in training mode, row softmax, row normalisation, token assembly, the
element-wise helpers, and the adjoints that have a kernel of their own.  A helper of tests/test_kernel_bounds_{cpu,gpu}.py,
imported through sys.path like tests/engine_bounds.py; it needs nothing but torch.

    reference(op, inp) -> (ref, bound)      float64 CPU tensors (tuples of them for an operation with several outputs)
    impl(op, inp, dtype, wrong=None)        the kernel's formula restated in torch in `dtype`: float32 = the independent fp32
                                            implementation that sets the margins; float64 + wrong = a structurally wrong variant

ref comes from torch's own float64 ops (F.interpolate, F.grid_sample, F.layer_norm, F.group_norm, F.batch_norm, torch.softmax,
F.normalize, F.avg_pool2d, and torch's float64 autograd of those for the adjoints), never from impl() and never from this
project's kernels.  bound = MARGIN[op] x model, u = 2^-24 (fp32 unit roundoff).  The models:

* Sampling (resize: align_corners=True, result times mul; warp: grid_sample with zeros padding after the reference's normalise /
  de-normalise round trip of the coordinate).  v = sum over 4 taps of w_t t:  a weight is a difference (1 rounding) and a product
  (1), each tap product rounds (1), three adds (<= 3 on the path), mul (1):  7 u S, S = sum w_t |t|.  The source coordinate is
  itself computed in fp32: resize fx = fl(fl((W-1)/(Wo-1)) ox): |dfx| <= 2 u |fx|;  warp ix = roundtrip(x + flow): the sum, the
  division, -1, +1 (absolute u of a value <= 1 + |n|, scaled back by (size-1)/2) and the last product: |dix| <= 4 u max(|ix|,
  size - 1).  A coordinate error moves the value by |dix| x the local slope in that direction, slope_x = wy0 |t01 - t00| + wy1
  |t11 - t10| with taps outside the image = 0 (the jump to zero at the border is a slope like any other: the padded bilinear
  surface is continuous).  When [ix - d, ix + d] contains an integer the fp32 coordinate may fall into the neighbouring interval;
  the value is continuous there and the slope is taken as the larger of the two intervals'.  This term dominates when smooth
  maps are up-sampled (2.8e-6 absolute at 16 -> 32) and is why a flat k u |y| is wrong here.
      model = |mul| u (7 S + cx slope_x + cy slope_y),   cx = 2 |fx| (resize), 4 max(|ix|, W - 1) (warp).
  Operand outputs (hl / h formats): + engine_bounds' activation-split model 2^-22 |v| + 2^-27 (2^-11 |v| + 2^-27 for one term).
* avgpool2: ((a + b) + (c + d)) / 4: two roundings on the path to each term, the scaling by 0.25 exact: 3 u (|a|+|b|+|c|+|d|) / 4.
* Two-pass normalisation over n elements (LayerNorm: a row; GroupNorm: HW x C/G of one image; a lane owns n/64 (n/256)
  elements in sequence and the lanes are folded by a butterfly): |dmean| <= cs u A, A = sum|x| / n, cs = log2(n) + 2 (the
  pairwise figure; a sequential lane sum random-walks below it for n <= 2^15).  d = x - mean rounds once; sum d^2 is insensitive
  to dmean in first order (sum d = 0), relative error (cs + 3) u, so rstd = 1/sqrt(var + eps) errs (cs/2 + 3.5) u relative.
      y = d rstd gamma + beta:   model = u (|gamma| rstd (cs A + (cs/2 + 7) |x - mean|) + |beta| + |y|).
  The first term is the conditioning: data with mean/std = 100 loses two digits, a row of constants (var = 0, rstd = eps^-1/2)
  shows the mean's rounding magnified by rstd.  ReLU is 1-Lipschitz.
* BatchNorm (training): the column sums of x and x^2 are accumulated in DOUBLE (bn_partial_kernel), mean / var / 1/sqrt in double:
  no n-dependent term.  scale = fl(gamma fl(rstd)), shift = fl(beta - fl(mean) scale), y = fma(x, scale, shift):
      model = u (3 |gamma| rstd (|x| + |mean|) + 2 |beta| + |y|)  + u |r| + u |y| per residual.
  running_mean / running_var (unbiased n / (n-1) there, biased in y): two products and a sum: 3 u (|(1-m) old| + |m new|).
* softmax: e = expf(x - max) — ROCm's ocml documents expf at 1 ulp (ROCm device-libs, ocml.md "Supported functions and ULP
  error": exp 1 ulp for fp32), the argument's own rounding adds u |x - max| relative: (2 + |x - max|) u; the sum of n positive
  terms cs u; one reciprocal and one product 2 u:   model = u p (6 + cs + |x - max|),  p exactly 0 beside -inf.
* normalize rows: n fma, sqrt, max, one division: model = u |q| (cs + 4), n <= 64.  assemble tokens, elementwise add / mul:
  one rounding, u |y|.  Activation forward: relu / leaky exact resp. 1 rounding; tanh 2^-22 absolute; gelu 2e-6 + 2^-23 |z| —
  the figures engine_bounds uses for the same device functions.
* Adjoints, ref = float64 autograd of the float64 forward.
  - softmax: ds = p (dp - s), s = sum p dp;  p arrives rounded to fp32 (u):  model = u |p| ((cs + 3) sum |p dp| + 5 (|dp| + |s|)).
  - normalize: dx = (dq - q (q . dq)) / |x|:  model = u (cs + 8) (|dq| + |q| sum |q dq|) / max(|x|, eps).
  - LayerNorm: xh errs e_xh = u (rstd cs A + (cs/2 + 5) |xh|);  a = mean(dh), b = mean(dh xh), dh = dy gamma:
      dx model = rstd (u (cs + 4) (|dh| + mean|dh| + |xh| mean|dh xh|) + |xh| mean(|dh| e_xh) + |b| e_xh) ;  gx = dy xh: |dy| e_xh + u |gx|.
      dgamma / dbeta are column sums (pp_colsum) of gx / dy: column-wise, below, plus the column sum of gx's own bound.
  - colsum over `rows` values: any order errs at most (rows - 1) u sum|x|, useless at 131 072 rows (8e-3); blocked sums of
    zero-mean gradients random-walk: sqrt(rows) u sum|x| is already generous (the kernel's longest chain is 64 + 32 + 22 adds) and
    still 2^-7 below a lost slab at 131 072 rows.  Column-wise (one number per column) because an element-wise model would need the tree.
  - resize: the transposed weights: model = |mul| u sum_o |dy_o| (7 w_o + 2 |fx| wy_o [x tap] + 2 |fy| wx_o [y tap]).
  - avgpool2: 0.25 dy, exact: bit-equal.  Activation: dy act'(z): 2^-22 |dy| (tanh, gelu'), exact otherwise.
  - GroupNorm (+ReLU): the LayerNorm model over the group's HW x C/G elements with dy masked by the ReLU; an element whose
    pre-activation lies within the forward bound of 0 may fall on either side of the mask: its |dy gamma| is added to its own dx
    and, through the two group means, to the others'; dgamma / dbeta column sums over B x HW rows as above.
  - BatchNorm (training, +ReLU): statistics and the channel sums dbeta = sum g, dgamma = sum g xh in double, mean and rstd handed
    on as fp32 (xh errs u (rstd (|x| + |mean|) + 2 |xh|)), dx evaluated in double from the double means and rounded once:
    dx model = |gamma| rstd (2 u (|g| + |mean g| + |xh mean(g xh)|) + |mean(g xh)| e_xh + (|xh| m_dgamma + m_dbeta) / rows) + u |dx|; no
    n-dependent term.  The same allowance for the ReLU mask.
  - warp: dfeat[q] = sum of contributions dy w; the atomics add in any order: (m + 4) u sum|contribution| with m the number of
    contributions to q, plus the coordinate term as in the forward.  dflow = sum_c dy (tap differences) x the other direction's
    weights: u (cs(C) + 8) sum_c |dy| (|t| ..) plus the coordinate term on the mixed difference; where the coordinate lies within
    1e-4 of an integer the gradient along THAT axis jumps and that component is held to a loose bound only (unclamped coordinates on
    axes longer than 1); a clamped coordinate has every tap invalid and along an axis of size 1 the coordinate does not depend on
    the flow: exactly 0 in both cases.
* Layout kernels (transpose / to_nhwc / to_nchw / tokens_to_nchw / gather_rows): no arithmetic, bit-equal to torch indexing; tested
  on the GPU only.

Margins.  MARGIN[op] = at most 4 x the worst |err| / model of impl(op, ., float32) over the whole sweep, measured on the CPU by
tests/test_kernel_bounds_cpu.py (which prints them); never from the HIP kernels.  The measured worst ratio and the margin of every
operation are the _set(op, measured, margin) calls below (and the table in DESIGN.md).  avgpool2_bwd is exact: margin 0 means
bit-equal.  assemble / elementwise are one rounding: the model is already the worst case.
The unbiased-variance error is 1 / (2n) relative; it is asserted only where it exceeds the bound's relative size:
separable_unbiased(op, n, offset):  1 / (2n) > 2 MARGIN u (cs (offset + 1) + cs/2 + 9)   (BatchNorm: 3 (2 offset + 1) + 3).
"""
import math

import torch
import torch.nn.functional as F

import engine_bounds as eb

U = 2.0 ** -24
TINY = 2.0 ** -126      # the smallest normal fp32 number: a probability below it is a subnormal (or flushed to zero)
check = eb.check
WORST = {}

# worst |err| / model of the fp32 CPU implementation over the sweep (test_kernel_bounds_cpu.py prints it) and the margin chosen (<= 4 x)
MEASURED = {}
MARGIN = {}


def _set(op, measured, margin):
    assert margin <= 4.0 * measured + 1e-12, (op, measured, margin)
    MEASURED[op], MARGIN[op] = measured, margin


_set("resize", 0.599, 1.9)
_set("warp", 0.339, 1.1)
_set("avgpool2", 0.645, 2.0)
_set("layernorm", 0.495, 1.8)
_set("groupnorm", 0.461, 1.5)
_set("batchnorm", 0.813, 2.6)
_set("softmax", 0.828, 2.7)
_set("normalize", 0.286, 0.9)
_set("assemble", 1.0, 1.0)
_set("act", 0.6, 1.9)
_set("elementwise", 1.0, 1.0)
_set("layernorm_bwd", 0.539, 1.7)
_set("softmax_bwd", 0.362, 1.15)
_set("normalize_bwd", 0.54, 1.7)
_set("resize_bwd", 0.447, 1.4)
_set("avgpool2_bwd", 0.0, 0.0)
_set("warp_bwd", 0.253, 0.8)
_set("colsum", 0.32, 1.0)
_set("act_bwd", 0.388, 1.2)
_set("groupnorm_bwd", 0.27, 0.9)
_set("batchnorm_bwd", 0.608, 1.9)


def cs(n):
    return math.log2(max(int(n), 1)) + 2.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _offset_data(g, shape, offset):
    """white noise of unit std around `offset` (mean / std = offset)"""
    return torch.randn(*shape, generator=g) + float(offset)


def _decades(g, n, lo=-2.0, hi=1.0):
    """n values with random sign whose sizes span 10^lo .. 10^hi"""
    m = 10.0 ** (torch.rand(n, generator=g) * (hi - lo) + lo)
    return m * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()


def _row_scales(g, n, decades):
    """n scales spanning 10^-decades .. 10^decades at random; the first is the smallest (std 10^-decades: where eps shows)"""
    s = 10.0 ** (torch.rand(n, generator=g) * 2 * decades - decades)
    s[0] = 10.0 ** -decades
    return s


# ------------------------------------------------------------------------------------------------------------------ the sweep
def _resize_cases():
    geo = [((16, 16), (32, 32)), ((32, 32), (64, 64)), ((5, 7), (9, 11)), ((64, 64), (37, 37)), ((1, 9), (1, 17)), ((9, 1), (4, 1)),
           ((8, 8), (1, 1)), ((8, 8), (8, 8))]
    Cs, muls, Bs = [1, 2, 6, 4, 12, 8, 256], [1.0, 2.0, -0.5], [1, 3]
    out = []
    for i, (hw, ho) in enumerate(geo):
        for j, C in enumerate(Cs):
            if C == 256 and hw[0] * ho[0] > 32 * 64:       # (the widest maps at the production sizes 16 -> 32 and 32 -> 64, not above)
                continue
            out.append(dict(H=hw[0], W=hw[1], Ho=ho[0], Wo=ho[1], C=C, mul=muls[(i + j) % 3], B=Bs[(i + j) % 2]))
    return out


def _warp_cases():
    out = []
    hws = [(8, 8), (16, 24), (1, 16), (64, 64), (3, 5)]
    Cs = [4, 8, 64, 256, 260, 512]
    k = 0
    for i, (H, W) in enumerate(hws):
        for j, C in enumerate(Cs):
            if (H, W) == (64, 64) and C not in (8, 256):
                continue
            B = 4 if (H, W) != (64, 64) else 2
            fb = [B, B // 2, 1][k % 3]
            out.append(dict(H=H, W=W, C=C, B=B, feat_batch=fb, ld_flow=[2, 4, 7][k % 3], kind="border"))
            k += 1
    out.append(dict(H=3, W=5, C=8, B=2, feat_batch=2, ld_flow=2, kind="integer"))
    out.append(dict(H=9, W=17, C=260, B=2, feat_batch=1, ld_flow=4, kind="integer"))
    return out


def _cross(*lists):
    out = [()]
    for l in lists:
        out = [a + (b,) for a in out for b in l]
    return out


CASES = {
    "resize": _resize_cases(),
    "warp": _warp_cases(),
    "avgpool2": [dict(C=C, H=H, W=W, B=[1, 5][(i + j) % 2]) for i, C in enumerate([1, 3, 64, 130])
                 for j, (H, W) in enumerate([(2, 2), (4, 6), (64, 64), (16, 2)])],
    "layernorm": [dict(rows=r, C=C, offset=[0, 10, 100][(i + j) % 3], const_row=(i + j) % 4 == 0 and r >= 3)
                  for i, r in enumerate([1, 3, 4, 5, 257, 8224]) for j, C in enumerate([1, 8, 24, 40, 100, 384, 512, 520, 768, 1000, 1024, 1032, 2048])],
    "groupnorm": [dict(B=B, HW=HW, C=C, G=G, relu=relu, offset=off)
                  for (B, HW, C, G) in [(2, 64, 256, 32), (1, 4096, 256, 32), (3, 15, 48, 4), (1, 1, 64, 32), (2, 100, 32, 32), (1, 300, 24, 1)]
                  for relu in (False, True) for off in (0, 10, 100)],
    "batchnorm": [dict(rows=r, C=C, relu=relu, res=res, offset=off)
                  for (r, C) in [(77, 64), (8192, 16), (2 * 64 * 64, 256), (3, 8), (2, 4)]
                  for (relu, res) in [(False, 0), (True, 0), (True, 1), (False, 2)] for off in (0, 10)],
    "softmax": [dict(rows=r, n=n, scale=[1.0, 30.0, 1e4][(i + j) % 3]) for i, n in enumerate([1, 2, 63, 64, 65, 257, 1025])
                for j, r in enumerate([1, 5, 1028])],
    "normalize": [dict(rows=r, n=n) for n in [1, 2, 3, 64] for r in [1, 9, 1000]],
    "assemble": [dict(T=T, C=C, B=2) for T in [1, 256, 1369] for C in [8, 384, 1000]],
    "act": [dict(n=n, act=a) for a in ["relu", "gelu", "leaky01", "tanh"] for n in [1, 255, 70001]],
    "elementwise": [dict(rows=r, cols=c, op=o) for o in (0, 1, 2) for (r, c) in [(1, 1), (7, 33), (300, 257)]],
    # adjoints: a small ragged shape and the production shape of the forward
    "layernorm_bwd": [dict(rows=r, C=C, offset=off) for (r, C, off) in [(5, 100, 0), (7, 40, 10), (50, 384, 0), (257, 1024, 10), (8224, 768, 0),
                                                                         (3, 520, 100), (66, 2048, 0), (1, 8, 0)]],
    "softmax_bwd": [dict(rows=r, n=n, scale=s) for (r, n, s) in [(1, 1, 1.0), (5, 2, 1.0), (5, 63, 30.0), (1028, 65, 1.0), (37, 257, 30.0), (9, 1025, 1.0)]],
    "normalize_bwd": [dict(rows=r, n=n) for n in [1, 2, 3, 64] for r in [1, 9, 1000]],
    "resize_bwd": [dict(H=5, W=7, Ho=9, Wo=11, C=3, mul=1.0, B=2), dict(H=32, W=32, Ho=64, Wo=64, C=256, mul=1.0, B=2),
                   dict(H=16, W=16, Ho=64, Wo=64, C=2, mul=2.0, B=3), dict(H=64, W=64, Ho=37, Wo=37, C=8, mul=-0.5, B=1),
                   dict(H=9, W=1, Ho=4, Wo=1, C=4, mul=1.0, B=1), dict(H=8, W=8, Ho=1, Wo=1, C=6, mul=2.0, B=2),
                   dict(H=1, W=9, Ho=1, Wo=17, C=12, mul=1.0, B=1), dict(H=8, W=8, Ho=8, Wo=8, C=8, mul=1.0, B=1)],
    "avgpool2_bwd": [dict(C=3, H=4, W=6, B=5), dict(C=64, H=64, W=64, B=1), dict(C=130, H=16, W=2, B=1), dict(C=1, H=2, W=2, B=1)],
    "warp_bwd": [dict(H=3, W=5, C=8, B=2), dict(H=1, W=16, C=8, B=2), dict(H=9, W=1, C=4, B=2), dict(H=8, W=8, C=16, B=2), dict(H=16, W=24, C=260, B=1), dict(H=64, W=64, C=256, B=2)],
    "colsum": [dict(rows=5, cols=3), dict(rows=131072, cols=768), dict(rows=8224, cols=384), dict(rows=63, cols=8), dict(rows=64, cols=260),
               dict(rows=1000, cols=1), dict(rows=4097, cols=1032), dict(rows=1, cols=4)],
    "act_bwd": [dict(n=n, act=a) for a in ["relu", "gelu", "leaky01", "tanh"] for n in [1, 255, 70001]],
    "groupnorm_bwd": [dict(B=3, HW=15, C=48, G=4, relu=False, offset=10), dict(B=2, HW=4096, C=256, G=32, relu=True, offset=0),
                      dict(B=2, HW=64, C=256, G=32, relu=True, offset=10), dict(B=1, HW=1, C=64, G=32, relu=False, offset=0),
                      dict(B=2, HW=100, C=32, G=32, relu=True, offset=0), dict(B=1, HW=300, C=24, G=1, relu=False, offset=100)],
    "batchnorm_bwd": [dict(rows=77, C=64, relu=False, res=0, offset=10), dict(rows=2 * 64 * 64, C=256, relu=True, res=0, offset=0),
                      dict(rows=8192, C=16, relu=True, res=0, offset=10), dict(rows=3, C=8, relu=False, res=0, offset=0),
                      dict(rows=2, C=4, relu=True, res=0, offset=0)],
}
OPS = list(CASES)


def case_name(op, c):
    return op + "(" + ",".join(f"{k}={v}" for k, v in c.items()) + ")"


def _upstream(g, shape):
    """an upstream gradient whose rows differ in size: every third row times 1e-3"""
    w = torch.randn(*shape, generator=g)
    w2 = w.view(-1, shape[-1]) if w.dim() > 1 else w.view(-1, 1)
    w2[::3] *= 1e-3
    return w


def border_flow(g, B, H, W, ld):
    """flows whose targets cover the 9 border situations: per axis the target lies in the left band (-1, 0) or the right band
    (size - 1, size) with probability 0.18 each, inside with 0.60 and beyond the image (all taps invalid) with 0.04: every edge
    ~11 %, every corner ~3 %, fully outside ~8 %"""
    def axis(size):
        u, k = torch.rand(B, H, W, generator=g), torch.rand(B, H, W, generator=g)
        inside = u * (size - 1)
        t = torch.where(k < 0.18, u - 1.0, torch.where(k < 0.36, size - 1 + u, inside))
        far = torch.where(u < 0.5, -1.0 - 3 * u, size + 3 * u)
        return torch.where(k >= 0.96, far, t)

    tx, ty = axis(W), axis(H)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    fl = torch.randn(B, H, W, ld, generator=g)
    fl[..., 0] = tx - xs
    fl[..., 1] = ty - ys
    return fl


def inputs(op, c, seed=0):
    g = _gen(1000 * OPS.index(op) + seed + sum(int(v * 7) if isinstance(v, (int, float)) else len(str(v)) for v in c.values()))
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    if op in ("resize", "resize_bwd"):
        d = dict(x=rn(c["B"], c["H"], c["W"], c["C"]))
        if op == "resize_bwd":
            d["dy"] = _upstream(g, (c["B"], c["Ho"], c["Wo"], c["C"]))
        return d
    if op == "warp":
        fl = border_flow(g, c["B"], c["H"], c["W"], c["ld_flow"])
        if c["kind"] == "integer":
            fl[..., :2] = torch.randint(-3, 4, (c["B"], c["H"], c["W"], 2), generator=g).float()
        return dict(feat=rn(c["feat_batch"], c["H"], c["W"], c["C"]), flow=fl)
    if op == "warp_bwd":
        return dict(feat=rn(c["B"], c["H"], c["W"], c["C"]), flow=border_flow(g, c["B"], c["H"], c["W"], 2),
                    dy=_upstream(g, (c["B"], c["H"], c["W"], c["C"])))
    if op in ("avgpool2", "avgpool2_bwd"):
        d = dict(x=rn(c["B"], c["H"], c["W"], c["C"]) + 0.5)
        if op == "avgpool2_bwd":
            d["dy"] = _upstream(g, (c["B"], c["H"] // 2, c["W"] // 2, c["C"]))
        return d
    if op in ("layernorm", "layernorm_bwd"):
        x = _offset_data(g, (c["rows"], c["C"]), c["offset"]) * _row_scales(g, c["rows"], 1.5).view(-1, 1)
        if c.get("const_row"):
            x[c["rows"] // 2] = 3.3
        d = dict(x=x, gamma=_decades(g, c["C"]), beta=rn(c["C"]))
        if op == "layernorm_bwd":
            d["dy"] = _upstream(g, (c["rows"], c["C"]))
        return d
    if op in ("groupnorm", "groupnorm_bwd"):
        x = _offset_data(g, (c["B"], c["HW"], c["C"]), c["offset"]) * _row_scales(g, c["B"], 1.0).view(-1, 1, 1)
        d = dict(x=x, gamma=_decades(g, c["C"]), beta=rn(c["C"]))
        if op == "groupnorm_bwd":
            d["dy"] = _upstream(g, (c["B"], c["HW"], c["C"]))
        return d
    if op in ("batchnorm", "batchnorm_bwd"):
        x = _offset_data(g, (c["rows"], c["C"]), c["offset"]) * _row_scales(g, c["C"], 1.0)
        d = dict(x=x, gamma=_decades(g, c["C"]), beta=rn(c["C"]), running_mean=rn(c["C"]), running_var=torch.rand(c["C"], generator=g) + 0.5)
        for i in range(c["res"]):
            d[f"res{i + 1}"] = rn(c["rows"], c["C"])
        if op == "batchnorm_bwd":
            d["dy"] = _upstream(g, (c["rows"], c["C"]))
        return d
    if op in ("softmax", "softmax_bwd"):
        x = rn(c["rows"], c["n"]) * c["scale"]
        if op == "softmax":
            if c["n"] > 2:
                x[0, 0:-1:3] = float("-inf")     # probability exactly 0 beside finite ones
            if c["scale"] >= 30:
                x[:, -1] = x.max(1).values + c["scale"]   # peaked rows peak in the last column, where a dropped tail shows
            if c["rows"] > 1:
                x[-1] = 0.75                      # a row of equal values
            return dict(x=x)
        return dict(x=x, dp=_upstream(g, (c["rows"], c["n"])))
    if op in ("normalize", "normalize_bwd"):
        x = rn(c["rows"], c["n"]) * (10.0 ** (torch.rand(c["rows"], 1, generator=g) * 4 - 2))
        if op == "normalize":
            x[0] *= 1e-10 / float(x[0].double().norm())   # norm 1e-10: where eps ADDED to the norm would show (1 %)
            if c["rows"] > 2:
                x[1] = 0.0                        # a zero row stays zero
                x[2] = 1e-20 / math.sqrt(c["n"])  # norm 1e-20: divided by eps
            return dict(x=x)
        return dict(x=x, dq=_upstream(g, (c["rows"], c["n"])))
    if op == "assemble":
        return dict(patches=rn(c["B"], c["T"], c["C"]), cls=rn(c["C"]), pos=rn(c["T"] + 1, c["C"]) * 3)
    if op in ("act", "act_bwd"):
        d = dict(z=rn(c["n"]) * 3)
        if op == "act_bwd":
            d["dy"] = _upstream(g, (c["n"],))
        return d
    if op == "elementwise":
        return dict(a=rn(c["rows"], c["cols"]), b=rn(c["rows"], c["cols"]), v=_decades(g, c["cols"]))
    if op == "colsum":
        return dict(x=_upstream(g, (c["rows"], c["cols"])))
    raise ValueError(op)


# ----------------------------------------------------------------------------------------------- bilinear taps (shared by impl and model)
def _tap(img, y, x, pad):
    """img (B, H, W, C); y, x integer (B, Ho, Wo) -> img[b, y, x] with the padding rule: zeros | clamp | wrap"""
    B, H, W, C = img.shape
    if pad == "wrap":
        yy, xx = y % H, x % W
        valid = None
    else:
        yy, xx = y.clamp(0, H - 1), x.clamp(0, W - 1)
        valid = ((y >= 0) & (y < H) & (x >= 0) & (x < W)) if pad == "zeros" else None
    bi = torch.arange(B).view(B, 1, 1).expand_as(yy)
    t = img[bi, yy, xx]
    if valid is not None:
        t = torch.where(valid.unsqueeze(-1), t, torch.zeros((), dtype=t.dtype))    # (an Inf / NaN behind an invalid tap never enters)
    return t


def _bilinear(img, iy, ix, pad, swap=False):
    """value (B, Ho, Wo, C) of the bilinear surface of img at (iy, ix) in img's dtype, with the taps and weights"""
    y0f, x0f = torch.floor(iy), torch.floor(ix)
    y0, x0 = y0f.long(), x0f.long()
    wx1, wy1 = ix - x0f, iy - y0f
    wx0, wy0 = (x0f + 1) - ix, (y0f + 1) - iy
    t00, t01, t10, t11 = _tap(img, y0, x0, pad), _tap(img, y0, x0 + 1, pad), _tap(img, y0 + 1, x0, pad), _tap(img, y0 + 1, x0 + 1, pad)
    e = lambda w: w.unsqueeze(-1)   # noqa: E731
    a0 = wx1 if swap else wx0       # the wrong variant: the first tap weighted lx where it should be 1 - lx
    v = e(wy0) * (e(a0) * t00 + e(wx1) * t01) + e(wy1) * (e(a0) * t10 + e(wx1) * t11)
    return v, (t00, t01, t10, t11), (wx0, wx1, wy0, wy1)


def _slopes(img, iy, ix, dy, dx, pad):
    """(S, slope_x dx + slope_y dy) in float64: the abs-weighted tap sum and the coordinate conditioning, the slope taken as the larger
    of the intervals that [i - d, i + d] touches"""
    _, (t00, t01, t10, t11), (wx0, wx1, wy0, wy1) = _bilinear(img, iy, ix, pad)
    e = lambda w: w.unsqueeze(-1)   # noqa: E731
    S = e(wy0) * (e(wx0) * t00.abs() + e(wx1) * t01.abs()) + e(wy1) * (e(wx0) * t10.abs() + e(wx1) * t11.abs())

    def sx_of(ixq):
        _, (a, b, c, d), (_, _, q0, q1) = _bilinear(img, iy, ixq, pad)
        return e(q0) * (b - a).abs() + e(q1) * (d - c).abs()

    def sy_of(iyq):
        _, (a, b, c, d), (p0, p1, _, _) = _bilinear(img, iyq, ix, pad)
        return e(p0) * (c - a).abs() + e(p1) * (d - b).abs()

    sx = torch.maximum(sx_of(ix - dx), sx_of(ix + dx))
    sy = torch.maximum(sy_of(iy - dy), sy_of(iy + dy))
    return S, sx * e(dx) + sy * e(dy)


def _resize_coords(c, dt, B):
    H, W, Ho, Wo = c["H"], c["W"], c["Ho"], c["Wo"]
    one = torch.ones((), dtype=dt)
    sy = (one * (H - 1)) / (one * (Ho - 1)) if Ho > 1 else one * 0
    sx = (one * (W - 1)) / (one * (Wo - 1)) if Wo > 1 else one * 0
    fy = (sy * torch.arange(Ho, dtype=dt)).view(1, Ho, 1).expand(B, Ho, Wo)
    fx = (sx * torch.arange(Wo, dtype=dt)).view(1, 1, Wo).expand(B, Ho, Wo)
    return fy, fx


def _warp_coords(c, flow, dt, wrong=None):
    B, H, W = flow.shape[:3]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")

    def rt(v, size):
        n = v * 2 / max(size - 1, 1) - 1
        return ((n + 1) / 2) * (size if wrong == "size" else size - 1)

    ix = rt(xs + flow[..., 0].to(dt), W)
    iy = rt(ys + flow[..., 1].to(dt), H)
    # (clamped two pixels outside, where every tap is invalid; fmaxf drops a NaN)
    ix = torch.nan_to_num(ix, nan=-2.0).clamp(-2.0, W + 1.0)
    iy = torch.nan_to_num(iy, nan=-2.0).clamp(-2.0, H + 1.0)
    return iy, ix


def _norm_view(op, c, t):
    """the tensor as (groups of statistics, n) and the function that undoes it"""
    if op.startswith("layernorm"):
        return t, (lambda r: r)
    B, HW, C, G = c["B"], c["HW"], c["C"], c["G"]
    cg = C // G
    v = t.view(B, HW, G, cg).permute(0, 2, 1, 3).reshape(B * G, HW * cg)
    return v, (lambda r: r.view(B, G, HW, cg).permute(0, 2, 1, 3).reshape(B, HW, C))


def _affine_view(op, c, p, shift=0):
    """gamma / beta laid out like _norm_view's rows (GroupNorm: one row of HW x cg per (image, group))"""
    if op.startswith("layernorm"):
        return p.view(1, -1)
    B, HW, C, G = c["B"], c["HW"], c["C"], c["G"]
    cg = C // G
    pg = p.view(G, cg)
    if shift:
        pg = torch.roll(pg, shift, 0)      # the wrong variant: the neighbouring group's channels
    return pg.view(1, G, 1, cg).expand(B, G, HW, cg).reshape(B * G, HW * cg)


EPS = {"layernorm": 1e-6, "layernorm_bwd": 1e-6, "groupnorm": 1e-5, "batchnorm": 1e-5, "groupnorm_bwd": 1e-5, "batchnorm_bwd": 1e-5}


# ------------------------------------------------------------------------------------------------------------- the formulas in torch
def impl(op, c, inp, dtype=torch.float32, wrong=None):
    """The operation as the kernel is specified to compute it, in `dtype`; wrong: the name of a structural error (WRONG[op])."""
    t = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in inp.items()}
    if op == "resize":
        x = t["x"]
        if wrong == "align_false":
            return c["mul"] * F.interpolate(x.permute(0, 3, 1, 2), size=(c["Ho"], c["Wo"]), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        fy, fx = _resize_coords(c, dtype, x.shape[0])
        v, _, _ = _bilinear(x, fy, fx, "clamp", swap=wrong == "weight_swapped")
        return v * c["mul"]
    if op == "warp":
        B = t["flow"].shape[0]
        feat = t["feat"][torch.arange(B) % c["feat_batch"]]
        iy, ix = _warp_coords(c, t["flow"], dtype, wrong)
        pad = {"border": "clamp", "wrap": "wrap"}.get(wrong, "zeros")
        return _bilinear(feat, iy, ix, pad, swap=wrong == "weight_swapped")[0]
    if op == "avgpool2":
        x = t["x"]
        a, b = x[:, 0::2, 0::2], x[:, 0::2, 1::2]
        cc, d = (x[:, 0::2, 1::2], x[:, 0::2, 1::2]) if wrong == "row_stride" else (x[:, 1::2, 0::2], x[:, 1::2, 1::2])  # W * C taken as C
        return ((a + b) + (cc + d)) * 0.25
    if op in ("layernorm", "groupnorm"):
        x, undo = _norm_view(op, c, t["x"])
        g, b = _affine_view(op, c, t["gamma"], 1 if wrong == "neighbour_group" else 0), _affine_view(op, c, t["beta"])
        n = x.shape[1]
        if wrong == "lost_tail":
            mean = x[:, :-1].sum(1, keepdim=True) / max(n - 1, 1)
        elif wrong == "padded_mean":     # C rounded up to 8; where that is the identity, to the zero-filled register slots of the kernel
            slots = 512 if n <= 512 else (1024 if n <= 1024 else -(-n // 64) * 64)
            mean = x.sum(1, keepdim=True) / (-(-n // 8) * 8 if n % 8 else slots)
        else:
            mean = x.sum(1, keepdim=True) / n
        d = x - mean
        var = (d * d).sum(1, keepdim=True) / (max(n - 1, 1) if wrong == "unbiased" else n)
        eps = EPS[op]
        rstd = 1.0 / (torch.sqrt(var) + eps) if wrong == "eps_outside" else 1.0 / torch.sqrt(var + eps)
        y = d * rstd * g + b
        if c.get("relu"):
            y = F.relu(y)
        return undo(y)
    if op == "batchnorm":
        x = t["x"]
        rows = x.shape[0]
        xd = x.double()                   # the statistics are accumulated in double by the kernel
        mean = xd.mean(0)
        var = ((xd * xd).mean(0) - mean * mean).clamp_min(0)
        nvar = var * rows / (rows - 1) if wrong == "unbiased" else var
        eps = EPS[op]
        rstd = 1.0 / (torch.sqrt(nvar) + eps) if wrong == "eps_outside" else 1.0 / torch.sqrt(nvar + eps)
        sc = t["gamma"] * rstd.to(dtype)
        sh = t["beta"] - mean.to(dtype) * sc
        y = x * sc + sh
        if c["relu"]:
            y = F.relu(y)
        for k in ("res1", "res2"):
            if k in t:
                y = y + t[k]
        m = 0.1
        unb = var if wrong == "running_biased" else var * rows / (rows - 1)
        rm = (1 - m) * t["running_mean"] + m * mean.to(dtype)
        rv = (1 - m) * t["running_var"] + m * unb.to(dtype)
        return y, rm, rv
    if op == "softmax":
        x = t["x"]
        e = torch.exp(x - x.max(1, keepdim=True).values)
        nn = (x.shape[1] // 64) * 64 if wrong == "tail_dropped" else x.shape[1]
        return e / e[:, :nn].sum(1, keepdim=True)
    if op == "normalize":
        x = t["x"]
        nrm = torch.sqrt((x * x).sum(1, keepdim=True))
        return x / (nrm + 1e-12 if wrong == "eps_added" else nrm.clamp_min(1e-12))
    if op == "assemble":
        B = t["patches"].shape[0]
        tok = torch.cat([t["cls"].view(1, 1, -1).expand(B, 1, -1), t["patches"]], 1)
        return tok + (torch.roll(t["pos"], 1, 0) if wrong == "pos_shifted" else t["pos"])
    if op == "act":
        if wrong == "negated_argument":
            return eb.ACT_F[c["act"]](-t["z"])
        return eb.ACT_F[c["act"]](t["z"])
    if op == "elementwise":
        if wrong == "op_swapped":           # a * b for a + b and the reverse; the column vector indexed by row
            return [t["a"] + t["b"], t["a"] * torch.roll(t["v"], 1), t["a"] * t["b"]][c["op"]]
        return [t["a"] * t["b"], t["a"] * t["v"], t["a"] + t["b"]][c["op"]]
    if op == "colsum":
        x = t["x"]
        if wrong == "last_block_skipped":
            return x[: (x.shape[0] - 1) // 64 * 64].sum(0)
        acc = torch.zeros(x.shape[1], dtype=dtype)          # slabs of 256 rows added in order, as the kernel's partial / final passes
        for blk in x.split(256):
            acc = acc + blk.sum(0)
        return acc
    if op == "layernorm_bwd":
        x, g, dy = t["x"], t["gamma"].view(1, -1), t["dy"]
        n = x.shape[1]
        mean = x.sum(1, keepdim=True) / n
        d = x - mean
        rstd = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / n + EPS[op])
        xh, dh = d * rstd, dy * g
        a, b = dh.sum(1, keepdim=True) / n, (dh * xh).sum(1, keepdim=True) / n
        dx = rstd * (dh - a) if wrong == "no_xhat_term" else rstd * (dh - a - xh * b)
        return dx, impl("colsum", c, dict(x=dy * xh), dtype), impl("colsum", c, dict(x=dy), dtype)
    if op == "groupnorm_bwd":
        x, undo = _norm_view(op, c, t["x"])
        g, b, dy = _affine_view(op, c, t["gamma"]), _affine_view(op, c, t["beta"]), _norm_view(op, c, t["dy"])[0]
        n = x.shape[1]
        mean = x.sum(1, keepdim=True) / n
        d = x - mean
        rstd = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / n + EPS[op])
        xh = d * rstd
        if c["relu"]:
            dy = torch.where(xh * g + b > 0, dy, torch.zeros((), dtype=dtype))
        dh = dy * g
        a, bb = dh.sum(1, keepdim=True) / n, (dh * xh).sum(1, keepdim=True) / n
        dx = rstd * (dh - a) if wrong == "no_xhat_term" else rstd * (dh - a - xh * bb)
        C = c["C"]
        return undo(dx), impl("colsum", c, dict(x=undo(dy * xh).reshape(-1, C)), dtype), impl("colsum", c, dict(x=undo(dy).reshape(-1, C)), dtype)
    if op == "batchnorm_bwd":
        x, dy, gam, bet = t["x"], t["dy"], t["gamma"], t["beta"]
        xd = x.double()                    # statistics and channel sums in double, as the kernels (bnb_stats / bnb_sums) accumulate them
        mean64 = xd.mean(0)
        rstd64 = 1.0 / torch.sqrt(((xd * xd).mean(0) - mean64 * mean64).clamp_min(0) + EPS[op])
        mean, rstd = mean64.to(dtype), rstd64.to(dtype)
        xh = (x - mean) * rstd
        if c["relu"]:
            dy = torch.where(xh * gam + bet > 0, dy, torch.zeros((), dtype=dtype))
        db, dg = dy.double().sum(0), (dy * xh).double().sum(0)
        rows = x.shape[0]
        xhd = (xd - mean.double()) * rstd.double()
        core = dy.double() - db / rows if wrong == "no_xhat_term" else dy.double() - db / rows - xhd * (dg / rows)
        return (gam.double() * rstd.double() * core).to(dtype), dg.to(dtype), db.to(dtype)
    if op == "softmax_bwd":
        p = torch.softmax(inp["x"].double(), 1).float().to(dtype)        # the kernel is handed fp32 probabilities
        dp = t["dp"]
        s = (p * dp).sum(1, keepdim=True)
        return p * dp if wrong == "no_sum_term" else p * (dp - s)
    if op == "normalize_bwd":
        x, dq = t["x"], t["dq"]
        nrm = torch.sqrt((x * x).sum(1, keepdim=True)).clamp_min(1e-12)
        q = x / nrm
        return dq / nrm if wrong == "no_projection" else (dq - q * (q * dq).sum(1, keepdim=True)) / nrm
    if op == "resize_bwd":
        x = t["x"].clone().requires_grad_(True)
        impl("resize", c, dict(x=x), dtype, wrong).backward(t["dy"])      # the transposed weights of the same formula, in `dtype`
        return x.grad
    if op == "avgpool2_bwd":
        dy = t["dy"]
        dx = torch.zeros_like(t["x"])
        for i in (0, 1):
            for j in (0, 1):
                dx[:, i::2, j::2] = (0.5 if wrong == "half" else 0.25) * dy
        return dx
    if op == "warp_bwd":
        feat, flow = t["feat"].clone().requires_grad_(True), t["flow"].clone().requires_grad_(True)
        B, H, W = flow.shape[:3]
        ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
        ix = ((xs + flow[..., 0]) * 2 / max(W - 1, 1) - 1 + 1) / 2 * (W - 1)
        iy = ((ys + flow[..., 1]) * 2 / max(H - 1, 1) - 1 + 1) / 2 * (H - 1)
        if wrong == "degenerate_axis_gradient":     # along an axis of size 1 the gradient handed on as if the coordinate still moved with the flow
            if W == 1:
                ix = ix.detach() + (flow[..., 0] - flow[..., 0].detach())
            if H == 1:
                iy = iy.detach() + (flow[..., 1] - flow[..., 1].detach())
        out = _bilinear(feat, iy.clamp(-2.0, H + 1.0), ix.clamp(-2.0, W + 1.0), "clamp" if wrong == "border" else "zeros")[0]
        out.backward(t["dy"])
        return feat.grad, flow.grad
    if op == "act_bwd":
        z = t["z"].clone().requires_grad_(True)
        eb.ACT_F[c["act"]](z).backward(t["dy"])
        if wrong == "grad_at_negated_argument":     # act'(-z): the other branch of relu / leaky, gelu' with the sign of its x phi(x) term flipped
            z2 = (-t["z"]).clone().requires_grad_(True)
            eb.ACT_F[c["act"]](z2).backward(t["dy"])
            return z2.grad
        return z.grad
    raise ValueError(op)


# -------------------------------------------------------------------------------------------------------------- references and models
def _split_bound(v, terms):
    return (2.0 ** -22 if terms == 2 else 2.0 ** -11) * v.abs() + eb.FLOOR_ACT


def model(op, c, inp):
    """(ref, model): torch's float64 result and the un-margined forward-error model (tuples for several outputs)."""
    d = {k: (v.double() if v.is_floating_point() else v) for k, v in inp.items()}
    if op == "resize":
        x = d["x"]
        ref = c["mul"] * F.interpolate(x.permute(0, 3, 1, 2), size=(c["Ho"], c["Wo"]), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        fy, fx = _resize_coords(c, torch.float64, x.shape[0])
        S, cond = _slopes(x, fy, fx, 2 * U * fy.abs(), 2 * U * fx.abs(), "clamp")
        return ref, abs(c["mul"]) * (7 * U * S + cond)
    if op == "warp":
        B, H, W = d["flow"].shape[:3]
        feat = d["feat"][torch.arange(B) % c["feat_batch"]]
        fl = d["flow"]
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        gx = (xs + fl[..., 0]) * 2 / max(W - 1, 1) - 1
        gy = (ys + fl[..., 1]) * 2 / max(H - 1, 1) - 1
        ref = F.grid_sample(feat.permute(0, 3, 1, 2), torch.stack([gx, gy], -1), mode="bilinear", padding_mode="zeros",
                            align_corners=True).permute(0, 2, 3, 1)
        iy, ix = _warp_coords(c, fl, torch.float64)
        dx = 4 * U * torch.maximum(ix.abs(), torch.full_like(ix, W - 1.0))
        dy = 4 * U * torch.maximum(iy.abs(), torch.full_like(iy, H - 1.0))
        S, cond = _slopes(feat, iy, ix, dy, dx, "zeros")
        return ref, 7 * U * S + cond
    if op == "avgpool2":
        x = d["x"].permute(0, 3, 1, 2)
        return F.avg_pool2d(x, 2).permute(0, 2, 3, 1), 3 * U * F.avg_pool2d(x.abs(), 2).permute(0, 2, 3, 1)
    if op in ("layernorm", "groupnorm"):
        x = d["x"]
        if op == "layernorm":
            ref = F.layer_norm(x, (c["C"],), d["gamma"], d["beta"], EPS[op])
        else:
            ref = F.group_norm(x.permute(0, 2, 1), c["G"], d["gamma"], d["beta"], EPS[op]).permute(0, 2, 1)
            if c["relu"]:
                ref = F.relu(ref)
        xv, undo = _norm_view(op, c, x)
        g, b = _affine_view(op, c, d["gamma"]), _affine_view(op, c, d["beta"])
        n = xv.shape[1]
        mean = xv.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(xv.var(1, unbiased=False, keepdim=True) + EPS[op])
        A = xv.abs().mean(1, keepdim=True)
        k = cs(n)
        m = U * (g.abs() * rstd * (k * A + (k / 2 + 7) * (xv - mean).abs()) + b.abs() + ((xv - mean) * rstd * g + b).abs())
        return ref, undo(m.expand_as(xv).contiguous())
    if op == "batchnorm":
        x = d["x"]
        rows = x.shape[0]
        rm, rv = d["running_mean"].clone(), d["running_var"].clone()
        y = F.batch_norm(x.t().unsqueeze(0), rm, rv, d["gamma"], d["beta"], True, 0.1, EPS[op])[0].t()
        mean, var = x.mean(0), x.var(0, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + EPS[op])
        m = U * (3 * d["gamma"].abs() * rstd * (x.abs() + mean.abs()) + 2 * d["beta"].abs() + y.abs())
        if c["relu"]:
            y = F.relu(y)
        for k in ("res1", "res2"):
            if k in d:
                y = y + d[k]
                m = m + U * (d[k].abs() + y.abs())
        unb = var * rows / (rows - 1)
        m_rm = 3 * U * (0.9 * d["running_mean"].abs() + 0.1 * mean.abs())
        m_rv = 3 * U * (0.9 * d["running_var"].abs() + 0.1 * unb.abs())
        return (y, rm, rv), (m, m_rm, m_rv)
    if op == "softmax":
        x = d["x"]
        p = torch.softmax(x, 1)
        dist = torch.nan_to_num(x.max(1, keepdim=True).values - x, posinf=0.0)
        return p, U * p * (6 + cs(x.shape[1]) + dist) + TINY
    if op == "normalize":
        q = F.normalize(d["x"], dim=1)
        return q, U * q.abs() * (cs(d["x"].shape[1]) + 4)
    if op == "assemble":
        B = d["patches"].shape[0]
        y = torch.cat([d["cls"].view(1, 1, -1).expand(B, 1, -1), d["patches"]], 1) + d["pos"]
        return y, U * y.abs()
    if op == "act":
        y = eb.ACT_F[c["act"]](d["z"])
        return y, 2 * U * y.abs() + eb.ACT_ERR[c["act"]] + (eb.EPI * d["z"].abs() if c["act"] == "gelu" else 0.0)
    if op == "elementwise":
        y = [d["a"] * d["b"], d["a"] * d["v"], d["a"] + d["b"]][c["op"]]
        return y, U * y.abs()
    if op == "colsum":
        x = d["x"]
        return x.sum(0), U * math.sqrt(x.shape[0]) * x.abs().sum(0)
    if op == "layernorm_bwd":
        x = d["x"].clone().requires_grad_(True)
        g, b = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
        F.layer_norm(x, (c["C"],), g, b, EPS[op]).backward(d["dy"])
        xv, dy, gv = d["x"], d["dy"], d["gamma"].view(1, -1)
        n = xv.shape[1]
        k = cs(n)
        mean = xv.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(xv.var(1, unbiased=False, keepdim=True) + EPS[op])
        xh, dh = (xv - mean) * rstd, dy * gv
        e_xh = U * (rstd * k * xv.abs().mean(1, keepdim=True) + (k / 2 + 5) * xh.abs())
        bb = (dh * xh).mean(1, keepdim=True)
        m_dx = rstd * (U * (k + 4) * (dh.abs() + dh.abs().mean(1, keepdim=True) + xh.abs() * (dh * xh).abs().mean(1, keepdim=True))
                       + xh.abs() * (dh.abs() * e_xh).mean(1, keepdim=True) + bb.abs() * e_xh)
        m_gx = dy.abs() * e_xh + U * (dy * xh).abs()
        rt = U * math.sqrt(xv.shape[0])
        m_dg = rt * (dy * xh).abs().sum(0) + m_gx.sum(0)
        m_db = rt * dy.abs().sum(0) + U * dy.sum(0).abs()
        return (x.grad, g.grad, b.grad), (m_dx, m_dg, m_db)
    if op == "groupnorm_bwd":
        x = d["x"].clone().requires_grad_(True)
        g, b = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
        y = F.group_norm(x.permute(0, 2, 1), c["G"], g, b, EPS[op]).permute(0, 2, 1)
        (F.relu(y) if c["relu"] else y).backward(d["dy"])
        C = c["C"]
        _, mf = model("groupnorm", dict(c, relu=False), dict(x=inp["x"], gamma=inp["gamma"], beta=inp["beta"]))
        flip = (y.detach().abs() <= MARGIN["groupnorm"] * mf) if c["relu"] else torch.zeros_like(mf, dtype=torch.bool)
        dym = torch.where(y.detach() > 0, d["dy"], torch.zeros_like(d["dy"])) if c["relu"] else d["dy"]
        xv, undo = _norm_view(op, c, d["x"])
        gv, dyv, fl = _affine_view(op, c, d["gamma"]), _norm_view(op, c, dym)[0], _norm_view(op, c, flip)[0]
        dyf = _norm_view(op, c, d["dy"].abs())[0] * fl            # a pre-activation within its own bound of 0 may take either side of the mask
        m_dx, m_gx = _norm_bwd_model(xv, dyv, gv, EPS[op], dyf)
        rt = U * math.sqrt(c["B"] * c["HW"])
        m_dg = rt * undo((dyv * _xhat(xv, EPS[op])).abs().contiguous()).reshape(-1, C).sum(0) + undo(m_gx.contiguous()).reshape(-1, C).sum(0)
        m_db = rt * dym.abs().reshape(-1, C).sum(0) + U * dym.reshape(-1, C).sum(0).abs() + undo(dyf.contiguous()).reshape(-1, C).sum(0)
        return (x.grad, g.grad, b.grad), (undo(m_dx.contiguous()), m_dg, m_db)
    if op == "batchnorm_bwd":
        x = d["x"].clone().requires_grad_(True)
        g, b = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
        y = F.batch_norm(x.t().unsqueeze(0), None, None, g, b, True, 0.1, EPS[op])[0].t()
        (F.relu(y) if c["relu"] else y).backward(d["dy"])
        rows = x.shape[0]
        (_, _, _), (mf, _, _) = model("batchnorm", dict(c, relu=False, res=0), {k: v for k, v in inp.items() if k not in ("dy", "res1", "res2")})
        flip = (y.detach().abs() <= MARGIN["batchnorm"] * mf) if c["relu"] else torch.zeros_like(mf, dtype=torch.bool)
        dym = torch.where(y.detach() > 0, d["dy"], torch.zeros_like(d["dy"])) if c["relu"] else d["dy"]
        xv, gam = d["x"], d["gamma"].abs()
        mean, rstd = xv.mean(0), 1.0 / torch.sqrt(xv.var(0, unbiased=False) + EPS[op])
        xh = (xv - mean) * rstd
        e_xh = U * (rstd * (xv.abs() + mean.abs()) + 2 * xh.abs())
        dyf = d["dy"].abs() * flip
        m_db = 2 * U * dym.sum(0).abs() + 2.0 ** -50 * dym.abs().sum(0) + dyf.sum(0)
        m_dg = U * (dym * xh).sum(0).abs() + (dym.abs() * e_xh).sum(0) + (dyf * xh.abs()).sum(0)
        mg, mgx = dym.mean(0), (dym * xh).mean(0)
        m_dx = gam * rstd * (2 * U * (dym.abs() + mg.abs() + (xh * mgx).abs()) + mgx.abs() * e_xh + xh.abs() * m_dg / rows + m_db / rows + dyf) + U * x.grad.abs()
        return (x.grad, g.grad, b.grad), (m_dx, m_dg, m_db)
    if op == "softmax_bwd":
        x = d["x"].clone().requires_grad_(True)
        p = torch.softmax(x, 1)
        p.backward(d["dp"])
        p, dp = p.detach(), d["dp"]
        s = (p * dp).sum(1, keepdim=True)
        return x.grad, (U * p + TINY) * ((cs(x.shape[1]) + 3) * (p * dp).abs().sum(1, keepdim=True) + 5 * (dp.abs() + s.abs()))
    if op == "normalize_bwd":
        x = d["x"].clone().requires_grad_(True)
        q = F.normalize(x, dim=1)
        q.backward(d["dq"])
        q, dq = q.detach(), d["dq"]
        nrm = d["x"].norm(dim=1, keepdim=True).clamp_min(1e-12)
        return x.grad, U * (cs(x.shape[1]) + 8) * (dq.abs() + q.abs() * (q * dq).abs().sum(1, keepdim=True)) / nrm
    if op == "resize_bwd":
        x = d["x"].clone().requires_grad_(True)
        (c["mul"] * F.interpolate(x.permute(0, 3, 1, 2), size=(c["Ho"], c["Wo"]), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)).backward(d["dy"])
        # the transposed |weights| and coordinate sensitivities: the adjoint of a forward whose taps carry those weights
        B = x.shape[0]
        fy, fx = _resize_coords(c, torch.float64, B)
        z = torch.zeros_like(d["x"]).requires_grad_(True)
        _, taps, (wx0, wx1, wy0, wy1) = _bilinear(z, fy, fx, "clamp")
        e = lambda w: w.unsqueeze(-1)   # noqa: E731
        ex, ey = e(2 * U * fx.abs()), e(2 * U * fy.abs())
        t00, t01, t10, t11 = taps
        fwd = 7 * U * (e(wy0) * (e(wx0) * t00 + e(wx1) * t01) + e(wy1) * (e(wx0) * t10 + e(wx1) * t11))
        fwd = fwd + ex * (e(wy0) * (t00 + t01) + e(wy1) * (t10 + t11)) + ey * (e(wx0) * (t00 + t10) + e(wx1) * (t01 + t11))
        fwd.backward(d["dy"].abs())
        return x.grad, abs(c["mul"]) * z.grad
    if op == "avgpool2_bwd":
        x = d["x"].clone().requires_grad_(True)
        F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).backward(d["dy"])
        return x.grad, torch.zeros_like(x.grad)          # 0.25 dy is exact: bit-equal
    if op == "act_bwd":
        z = d["z"].clone().requires_grad_(True)
        eb.ACT_F[c["act"]](z).backward(d["dy"])
        smooth = c["act"] in ("gelu", "tanh")
        return z.grad, d["dy"].abs() * ((2.0 ** -22 + 2e-6 * (c["act"] == "gelu")) if smooth else U)
    if op == "warp_bwd":
        feat, fl = d["feat"].clone().requires_grad_(True), d["flow"].clone().requires_grad_(True)
        B, H, W, C = feat.shape
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        gx = (xs + fl[..., 0]) * 2 / max(W - 1, 1) - 1
        gy = (ys + fl[..., 1]) * 2 / max(H - 1, 1) - 1
        F.grid_sample(feat.permute(0, 3, 1, 2), torch.stack([gx, gy], -1), mode="bilinear", padding_mode="zeros",
                      align_corners=True).permute(0, 2, 3, 1).backward(d["dy"])
        iy, ix = _warp_coords(c, d["flow"], torch.float64)
        ddx = 4 * U * torch.maximum(ix.abs(), torch.full_like(ix, W - 1.0))
        ddy = 4 * U * torch.maximum(iy.abs(), torch.full_like(iy, H - 1.0))
        z = torch.zeros_like(d["feat"]).requires_grad_(True)
        _, (t00, t01, t10, t11), (wx0, wx1, wy0, wy1) = _bilinear(z, iy, ix, "zeros")
        e = lambda w: w.unsqueeze(-1)   # noqa: E731
        contrib = e(wy0) * (e(wx0) * t00 + e(wx1) * t01) + e(wy1) * (e(wx0) * t10 + e(wx1) * t11)
        count = t00 + t01 + t10 + t11
        sens = e(ddx) * (e(wy0) * (t00 + t01) + e(wy1) * (t10 + t11)) + e(ddy) * (e(wx0) * (t00 + t10) + e(wx1) * (t01 + t11))
        ga, = torch.autograd.grad(contrib, z, d["dy"].abs(), retain_graph=True)
        gm, = torch.autograd.grad(count, z, torch.ones_like(d["dy"]), retain_graph=True)
        gs, = torch.autograd.grad(sens, z, d["dy"].abs())
        m_feat = U * (gm + 4) * ga + gs
        # dflow
        fe = d["feat"]
        _, (a, b, cc, dd), _ = _bilinear(fe, iy, ix, "zeros")
        ady = d["dy"].abs()
        k = U * (cs(C) + 8)
        m_gx = k * (ady * (e(wy0) * (a.abs() + b.abs()) + e(wy1) * (cc.abs() + dd.abs()))).sum(-1) + ddy * (ady * ((b - a) - (dd - cc)).abs()).sum(-1)
        m_gy = k * (ady * (e(wx0) * (a.abs() + cc.abs()) + e(wx1) * (b.abs() + dd.abs()))).sum(-1) + ddx * (ady * ((b - a) - (dd - cc)).abs()).sum(-1)
        # the x gradient jumps where ix crosses an integer (its own axis only; the other component is continuous there), and only for a
        # coordinate that is not clamped (the clamped ones, -2 and size + 1, are integers whose taps are all invalid: exactly 0, which the
        # model above already says, every tap being 0) and on an axis with more than one pixel.  Along an axis of size 1 the coordinate
        # does not depend on the flow: the gradient is exactly 0.
        near = lambda v, size: ((v - torch.round(v)).abs() < 1e-4) & (v > -1.5) & (v < size + 0.5) & (size > 1)   # noqa: E731
        loose = (ady * (a.abs() + b.abs() + cc.abs() + dd.abs())).sum(-1) * 4 + float(ady.max()) * float(fe.abs().max()) * C
        m_gx = torch.where(near(ix, W), loose, m_gx + near(iy, H) * ddy * loose)
        m_gy = torch.where(near(iy, H), loose, m_gy + near(ix, W) * ddx * loose)
        if W == 1:
            m_gx = torch.zeros_like(m_gx)
        if H == 1:
            m_gy = torch.zeros_like(m_gy)
        m_fl = torch.stack([m_gx, m_gy], -1)
        return (feat.grad, fl.grad), (m_feat, m_fl)
    raise ValueError(op)


def _xhat(xv, eps):
    return (xv - xv.mean(1, keepdim=True)) / torch.sqrt(xv.var(1, unbiased=False, keepdim=True) + eps)


def _norm_bwd_model(xv, dyv, gv, eps, dyf):
    """(model of dx, model of gx = dy xhat) of the two-pass normalisation adjoint on rows of statistics; dyf: |dy| where the ReLU mask
    may fall on either side"""
    n = xv.shape[1]
    k = cs(n)
    rstd = 1.0 / torch.sqrt(xv.var(1, unbiased=False, keepdim=True) + eps)
    xh, dh = _xhat(xv, eps), dyv * gv
    e_xh = U * (rstd * k * xv.abs().mean(1, keepdim=True) + (k / 2 + 5) * xh.abs())
    bb = (dh * xh).mean(1, keepdim=True)
    dhf = dyf * gv.abs()
    m_dx = rstd * (U * (k + 4) * (dh.abs() + dh.abs().mean(1, keepdim=True) + xh.abs() * (dh * xh).abs().mean(1, keepdim=True))
                   + xh.abs() * (dh.abs() * e_xh).mean(1, keepdim=True) + bb.abs() * e_xh
                   + dhf + dhf.mean(1, keepdim=True) + xh.abs() * (dhf * xh.abs()).mean(1, keepdim=True))
    m_gx = dyv.abs() * e_xh + U * (dyv * xh).abs() + dyf * xh.abs()
    return m_dx, m_gx


def reference(op, c, inp, terms=0):
    """(ref, bound) = (torch's float64 result, MARGIN[op] x model); terms: 2 / 1 adds the operand-format split of the result."""
    ref, m = model(op, c, inp)
    k = MARGIN[op]
    if isinstance(ref, tuple):
        return ref, tuple(k * t for t in m)
    b = k * m
    if terms:
        b = b + _split_bound(ref, terms)
    return ref, b


def worst_ratio(got, ref, m):
    """worst |got - ref| / m over all outputs (0 / 0 counts as 0)"""
    if not isinstance(ref, tuple):
        got, ref, m = (got,), (ref,), (m,)
    w = 0.0
    for a, r, b in zip(got, ref, m):
        err = (a.detach().double() - r).abs()
        ratio = torch.where(err > 0, err / b.clamp_min(1e-300), torch.zeros_like(err))
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        if ratio.numel():
            w = max(w, float(ratio.max()))
    return w


def separable_unbiased(op, n, offset):
    """the n / (n - 1) variance error (1 / (2n) relative) exceeds twice the bound's relative size at |xhat| ~ 1"""
    k = cs(n)
    rel = (3 * (2 * offset + 1) + 3) if op == "batchnorm" else (k * (offset + 1) + k / 2 + 9)
    return n > 1 and 1.0 / (2 * n) > 2 * MARGIN[op] * U * rel


# wrong implementation -> the size rule under which a case contains its error (the case dict, n = elements per statistic)
def _n_of(op, c):
    return c["C"] if op.startswith("layernorm") else (c["HW"] * (c["C"] // c["G"]) if op.startswith("groupnorm") else c["rows"])


WRONG = {
    "resize": {
        "align_false": lambda c: (c["Ho"], c["Wo"]) != (c["H"], c["W"]),          # identity resampling has no interpolation
        "weight_swapped": lambda c: c["W"] > 1,
    },
    "warp": {
        "border": lambda c: True, "wrap": lambda c: True,
        "size": lambda c: True,
        "weight_swapped": lambda c: True,
    },
    "avgpool2": {"row_stride": lambda c: True},
    "layernorm": {
        "unbiased": lambda c: separable_unbiased("layernorm", c["C"], c["offset"]),
        "eps_outside": lambda c: c["C"] > 1,                                        # (row 0 has std 10^-1.5: eps / std against eps / (2 var))
        "lost_tail": lambda c: separable_unbiased("layernorm", c["C"], c["offset"]),
        # (no padding where C is a multiple of 8 AND fills the instance's register slots: 512 per lane group, 64 lanes in the any-width path)
        "padded_mean": lambda c: c["C"] % 8 != 0 or c["C"] != (512 if c["C"] <= 512 else (1024 if c["C"] <= 1024 else -(-c["C"] // 64) * 64)),
    },
    "groupnorm": {
        "unbiased": lambda c: separable_unbiased("groupnorm", _n_of("groupnorm", c), c["offset"]),
        "eps_outside": lambda c: _n_of("groupnorm", c) > 1,
        "lost_tail": lambda c: separable_unbiased("groupnorm", _n_of("groupnorm", c), c["offset"]), "neighbour_group": lambda c: c["G"] > 1,
    },
    "batchnorm": {
        "unbiased": lambda c: separable_unbiased("batchnorm", c["rows"], c["offset"]),
        "running_biased": lambda c: True, "eps_outside": lambda c: True,
    },
    "softmax": {"tail_dropped": lambda c: c["n"] % 64 != 0},
    "normalize": {"eps_added": lambda c: True},
    "assemble": {"pos_shifted": lambda c: True},
    "colsum": {"last_block_skipped": lambda c: c["rows"] > 1},
    "layernorm_bwd": {"no_xhat_term": lambda c: c["C"] > 1},
    "softmax_bwd": {"no_sum_term": lambda c: c["n"] > 1},
    "normalize_bwd": {"no_projection": lambda c: c["n"] > 1},
    "resize_bwd": {"align_false": lambda c: (c["Ho"], c["Wo"]) != (c["H"], c["W"]), "weight_swapped": lambda c: c["W"] > 1},
    "avgpool2_bwd": {"half": lambda c: True},
    "warp_bwd": {"border": lambda c: True},
    "groupnorm_bwd": {"no_xhat_term": lambda c: _n_of("groupnorm_bwd", c) > 1},
    "batchnorm_bwd": {"no_xhat_term": lambda c: True},
    "act": {"negated_argument": lambda c: True},
    "elementwise": {"op_swapped": lambda c: c["op"] != 1 or c["cols"] > 1},
    "act_bwd": {"grad_at_negated_argument": lambda c: c["act"] != "tanh"},        # (tanh' is even)
}
