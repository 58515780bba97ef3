"""Float64 references and element-wise error bounds for the Winograd transforms (csrc/pp_winograd.hip: F(2x2, 3x3) of the strict-fp32 mode,
F(4x4, 3x3) of the f16x3 engine, their chained forms) and the narrow predict layers (conv_narrow_kernel in csrc/pp_sample.hip).  A helper of
tests/test_wino_bounds_{cpu,gpu}.py, imported through sys.path like tests/corr_bounds.py; needs torch only.

    inputs(op, case)                          fp32 CPU tensors
    reference(op, case, inp) -> (ref, bound)  float64 CPU tensors, bound = MARGIN[op] x model
    impl(op, case, inp, dtype, wrong=None)    the kernels' expression order restated in torch in `dtype`: float32 sets the margins,
                                              float64 + wrong is a structurally wrong variant
    model(op, case, inp) -> (ref, model)      the un-margined model

ref comes from torch's float64 ops and float64 products with the textbook matrices, as the kernels' comments state them (wino_bt_d_b,
PP_W4_BT, the G of wino_weight_kernel / g6, PP_W4_AT): never from impl() or this project's kernels.  Layouts are the kernels': maps NHWC,
U (t^2, P, C) and Y (t^2, P, Cout) with frequency xi = t a + b and tile p = (b th + ty) tw + tx, th = H / m, tw = W / m, t = m + 2.

Stage ops and their models, u = 2^-24; a rounding count k is the longest chain of rounded operations on a path from an input to an output
of ONE 1-D pass, counted from the kernel's expression order, summed over the two passes (first order; a fused multiply-add only removes
roundings):
* in2  U = B^T d B per 4x4 tile, zero padding, optional ReLU first.  wino_bt_d_b: one add per pass: k_in2 = 2.  model = 2 u |B^T| |d| |B|.
* in4  the same per 6x6 tile on the OPERAND'S VALUES x = (hi + lo) / 4, output the operand's values (hi + lo) x 16.  PP_W4_BT: 4 d0 - 5 d2 + d4 is
  one rounded product (x 4, x 2 are exact) and two adds: 3 per pass, k_in4 = 6.  The result is split at scale 1 / 16: a = U / 16, hi = f16(a),
  lo = f16(a - hi): |a - hi - lo| <= 2^-22 |a| while lo is normal, else the subnormal grid 2^-24 of a, i.e. <= 2^-25 in a = 2^-21 in U
  (engine_bounds derives FLOOR_ACT = 2^-27 the same way at scale 4).  model = 6 u |B^T| |d| |B| + 2^-22 |U| + 2^-21.
  A tile whose window is all zero, and every input <= 0 under ReLU, gives EXACTLY 0: the model is 0 where |B^T| |d| |B| is.
* wt2  V = G g G^T.  0.5 (g0 +- g1 + g2): two adds per pass (x 0.5 exact): k_w2 = 4.
* wt4  g6: (1/24) g0 + (1/12) g1 + (1/6) g2: the constant rounds once, the product once, two adds: k_w4 = 8.
* out2 act(A^T Y A + bias) + r1 + r2: (y0 + y1) + y2: two adds per pass, k_out2 = 4.  The bias, the activation's output and each residual are
  charged engine_bounds.EPI of their size (+ u of the running sum per residual add); Lipschitz constant 1 (none / relu / leaky01).
* out4 (d12 + 8 d34) + y5: three adds per pass, k_out4 = 6.  Operand output: + 2^-22 |v| + 2^-27, the activation split of engine_bounds, of
  max(v, 0) with c_relu.
* narrow  conv_narrow_kernel multiplies the layer's fp32 filters into fp32 accumulators with fmaf, channels ascending inside a tap, taps
  row-major, 32-channel slices outermost; its hl input is summed hi + lo to the exact fp32 value 4 x once per staged element and the
  accumulator is scaled by 1 / 4 (exact).  So the operand rounding belongs to the input side only: ref = engine_bounds.reference("conv2d", ...,
  mode="f32") on the operand's values (hl input) or on the fp32 map, no floors.
* chain2 / chain4  U1 = in(out(Y)) of the chained kernels: the out bound carried through |B^T| . |B|, plus the in model of the float64 hidden map.
End to end, conv_w2 / conv_w4 (pair4: two layers on one input): ref = F.conv2d in float64 on the values the kernel reads,
    model = (k u + tau) A_w + floors, then the epilogue as above,  k = k_in + k_w + k_out (12 for F(2x2), 20 for F(4x4)), tau = engine_bounds.TAU,
    A_w = |A^T| [ sum_ci (|G| |g| |G^T|) .* (|B^T| |d| |B|) ] |A|: the Winograd pipeline on absolute values with absolute matrices (over the sweep
    a median of 7-12 x the direct |x| (x) |w| for F(2x2) and 60-70 x for F(4x4), more where the padding cancels taps: the price of the
    algorithm, not slack), floors (conv_w4): engine_bounds.floor_w(V) per weight
    element and 2^-21 per U element, through the same pipeline.

Margins: MARGIN[op] <= 4 x the worst |impl_fp32 - ref| / model over the sweep (for in4 / conv_w4 / chain4 the emulated operand arithmetic: hi / lo
fp16 split at the stated scales, fp32 accumulation), measured on the CPU by tests/test_wino_bounds_cpu.py, never from the HIP kernels.  They
sit at about 3 x the measured value; impl() uses element-wise torch ops only (the products one channel at a time), so the measured ratios
do not depend on the host's thread count.  bound = MARGIN x model + fixed (model()): the epilogue terms of an end-to-end op or of narrow
carry the margin of the output stage (out2 / out4: the same adds, the same operand split) and are taken off the error before the
contraction's ratio is measured, so that an epilogue-only case (a dead input, a zero tile) does not set the contraction's margin; a chain's
bound is composed of the stages' margins (the out bound of the hidden map carried through |B^T| . |B|, plus in's) and the pair takes conv_w4's.
"""
import torch
import torch.nn.functional as F

import engine_bounds as eb
import kernel_bounds as kb

U = kb.U
check = eb.check
worst_ratio = kb.worst_ratio
MEASURED, MARGIN = {}, {}
SPLIT_REL, FLOOR_U = 2.0 ** -22, 2.0 ** -21
K_IN, K_W, K_OUT = {2: 2, 4: 6}, {2: 4, 4: 8}, {2: 4, 4: 6}


def _set(op, measured, margin):
    assert margin <= 4.0 * measured + 1e-12, (op, measured, margin)
    MEASURED[op], MARGIN[op] = measured, margin


_set("in2", 0.887, 2.6)
_set("in4", 0.999, 3.0)
_set("wt2", 0.495, 1.5)
_set("wt4", 0.452, 1.35)
_set("out2", 0.393, 1.2)
_set("out4", 0.886, 2.6)
_set("narrow", 0.0862, 0.28)
_set("conv_w2", 0.00651, 0.02)
_set("conv_w4", 0.0501, 0.16)

_t = lambda rows: torch.tensor(rows, dtype=torch.float64)   # noqa: E731
BT = {2: _t([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]),
      4: _t([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]])}
G = {2: _t([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]),
     4: _t([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]])}
AT = {2: _t([[1, 1, 1, 0], [0, 1, -1, -1]]),
      4: _t([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]])}

# ------------------------------------------------------------------------------------------------------------------ the sweep
# (B, H, W, Cin, Cout): the smallest shapes that take each branch
F2 = [(1, 2, 2, 4, 32),        # one tile, every border
      (1, 2, 6, 4, 33),        # one tile row, H != W, scalar (non-VEC) output kernel
      (3, 6, 2, 8, 32),        # one tile column, batch decode
      (2, 8, 16, 36, 64),      # Cin % 4 only; chain eligible
      (1, 16, 16, 8, 32),      # P = 64: sixteen single launches
      (4, 16, 16, 8, 32)]      # P = 256: grouped launch
F4 = [(1, 4, 4, 8, 8),         # one tile
      (1, 4, 12, 8, 40),       # Cout % 8 only, H != W
      (3, 12, 4, 16, 8),       # one tile column, batch decode
      (2, 8, 16, 32, 32),      # small multi-tile, H != W
      (1, 64, 64, 8, 8),       # P = 256 exactly: no pad rows
      (17, 16, 16, 8, 8)]      # P = 272 -> 512: 240 pad rows
# chains (B, H, W, C): th = 1 (the ring never fills), th = 5 (the four-slot ring wraps), W = 32, W = 64 (F(4x4): NB = 2) at one tile row, ...
CHAIN2 = [(1, 2, 16, 32), (2, 10, 16, 64), (1, 4, 32, 32), (1, 2, 64, 32)]
CHAIN4 = [(1, 4, 16, 32), (2, 20, 16, 32), (1, 8, 32, 64), (1, 4, 64, 32), (1, 12, 64, 32)]
KINDS = ("randn", "decades", "offset", "const", "sparse", "impulse")
# epilogue variants, rotated over the cases: bias, act, residuals (F(2x2): + relu_in)
EPIS = [dict(bias=True, act="relu", nres=0), dict(bias=False, act=None, nres=2), dict(bias=True, act="leaky01", nres=1),
        dict(bias=True, act=None, nres=0), dict(bias=False, act="relu", nres=1)]
# F(4x4) outputs: fp32 map | operand (with / without the consumer's ReLU) | fp32 map + attached operand
OUTS4 = [dict(hl=False), dict(hl=True, c_relu=True), dict(hl=True, c_relu=False), dict(hl=False, also="relu")]


def _img_cases(fam):
    """every kind on the single-tile, the non-square and the batch-decode case; two kinds, rotating, on the rest; `dead` where a ReLU reads"""
    out = []
    for i, (B, H, W, Ci, Co) in enumerate(F2 if fam == 2 else F4):
        kinds = KINDS if i < 3 else [KINDS[(2 * i + j) % 5] for j in range(2)]
        for j, kind in enumerate(kinds):
            out.append(dict(B=B, H=H, W=W, Cin=Ci, Cout=Co, kind=kind, relu_in=(fam == 2 and (i + j) % 3 == 0)))
        if i < 4:
            out.append(dict(B=B, H=H, W=W, Cin=Ci, Cout=Co, kind="dead", relu_in=True))
    return out


def _cases():
    cs = {}
    for fam in (2, 4):
        img = _img_cases(fam)
        cs[f"in{fam}"] = [dict(B=c["B"], H=c["H"], W=c["W"], C=c["Cin"], kind=c["kind"], relu=c["relu_in"] or (fam == 4 and i % 4 == 1))
                          for i, c in enumerate(img)]
        cs[f"wt{fam}"] = [dict(Cout=co, Cin=ci, kind=k) for (co, ci) in ((8, 8), (33, 4), (40, 36)) for k in ("randn", "decades", "offset", "impulse")]
        outs = []
        chains = CHAIN2 if fam == 2 else CHAIN4
        geo = [(B, H, W, Co) for (B, H, W, _, Co) in (F2 if fam == 2 else F4)[:4]] + chains[:2]
        for i, (B, H, W, C) in enumerate(geo):
            for j, kind in enumerate(KINDS[:5] if i < 2 else [KINDS[(i + j) % 5] for j in range(2)]):
                c = dict(B=B, H=H, W=W, C=C, kind=kind, **EPIS[(i + j) % 5])
                if fam == 4:
                    c.update(OUTS4[(i + j) % 3])
                    if c["hl"]:
                        c["nres"] = 0
                        if C % 8:
                            c["hl"] = False
                outs.append(c)
        cs[f"out{fam}"] = outs
        cs[f"chain{fam}"] = [dict(B=B, H=H, W=W, C=C, kind=KINDS[(i + j) % 5], bias=(i + j) % 2 == 0, act=(None, "relu", "leaky01")[(i + j) % 3],
                                  c_relu=(i + j) % 2 == 1) for i, (B, H, W, C) in enumerate(chains) for j in range(2)]
        conv = []
        for i, c in enumerate(img):
            if fam == 4 and c["kind"] == "dead":            # (the operand's producer applies the input ReLU: in4 alone has the flag)
                continue
            e = dict(c, **EPIS[i % 5])
            if fam == 4:
                e.update(OUTS4[i % 4])
                if e["hl"]:
                    e["nres"] = 0
            if c["kind"] == "dead":
                e["nres"] = 2 if not e.get("hl") else 0
            conv.append(e)
        cs[f"conv_w{fam}"] = conv
    cs["pair4"] = [dict(B=B, H=H, W=W, Cin=Ci, Ca=16, Cb=8, kind=k, bias=True, act="relu", hl=True, c_relu=cr, nres=0, relu_in=False)
                   for (B, H, W, Ci) in ((1, 4, 12, 8), (2, 8, 16, 32)) for (k, cr) in (("randn", True), ("decades", False))]
    cs["narrow"] = [dict(B=B, H=m * (256 // W), W=W, C=32, k=k, Cout=co, hl=hl, kind=KINDS[(W // 16 + k + co + m + B) % 5], res=(k + co + B) % 2 == 0)
                    for W in (16, 32, 64) for m in (1, 2) for (k, co, B) in ((1, 1, 1), (3, 2, 3), (3, 1, 1), (1, 2, 3)) for hl in (True, False)]
    return cs


def case_name(op, c):
    return op + "(" + ",".join(f"{k}={v}" for k, v in c.items()) + ")"


def fam_of(op):
    return 2 if op.endswith("2") else 4


# ------------------------------------------------------------------------------------------------------------------ data
def _fill(kind, shape, g):
    """a tensor whose LAST axis is the channels"""
    C = shape[-1]
    if kind in ("randn", "impulse"):
        return torch.randn(*shape, generator=g)
    if kind == "decades":                                   # channel c scaled by 10^(-3 .. 2)
        return torch.randn(*shape, generator=g) * 10.0 ** torch.linspace(-3, 2, C)
    if kind == "offset":                                    # mean 100, std 1: the transforms cancel the mean
        return torch.randn(*shape, generator=g) + 100.0
    if kind == "const":                                     # the borders are the only structure
        return torch.full(shape, 1.7) * (1.0 + torch.arange(C) % 3)
    if kind == "sparse":                                    # 5 % non-zero: whole tiles are zero
        return torch.randn(*shape, generator=g) * (torch.rand(*shape[:-1], 1, generator=g) < 0.05)
    if kind == "dead":                                      # all <= 0: nothing passes the input ReLU
        return -torch.randn(*shape, generator=g).abs()
    raise ValueError(kind)


def impulse_pixels(H, W, m):
    """the four corners and the four pixels around the first interior tile corner"""
    px = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)] + [(y, x) for y in (m - 1, m) for x in (m - 1, m) if y < H and x < W]
    return sorted(set(px))


def _image(kind, B, H, W, C, m, g):
    if kind != "impulse":
        return _fill(kind, (B, H, W, C), g)
    x = torch.zeros(B, H, W, C)
    for i, (y, xx) in enumerate(impulse_pixels(H, W, m)):
        x[:, y, xx, i % C] = 1.0 + i
    return x


def _weight(kind, Cout, Cin, g):
    if kind == "impulse":                                   # one-hot tap (ky, kx) = (0, 2) of channel co % Cin: out[y, x, co] = x[y - 1, x + 1, co % Cin]
        w = torch.zeros(Cout, Cin, 3, 3)
        w[torch.arange(Cout), torch.arange(Cout) % Cin, 0, 2] = 1.0
        return w
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    if kind == "decades":
        w = w * 10.0 ** torch.linspace(-2, 1, Cout).view(-1, 1, 1, 1)
    if kind == "offset":
        w = w + 0.5
    return w


def quantise(x, scale=4.0):
    """the values (hi + lo) / scale of the hl operand of x: hi = f16(scale x), lo = f16(scale x - hi)"""
    a = x.float() * scale
    hi = a.half().float()
    return ((hi + (a - hi).half().float()) / scale).to(x.dtype)


def inputs(op, c, seed=0):
    g = kb._gen(4100 + 97 * OPS.index(op) + seed + sum(int(v) * 5 if isinstance(v, (int, bool)) else len(str(v)) for v in c.values()))
    fam = fam_of(op) if op != "narrow" else 4
    m = fam
    d = {}
    if op in ("in2", "in4"):
        x = _image(c["kind"], c["B"], c["H"], c["W"], c["C"], m, g)
        return dict(x=quantise(x) if fam == 4 else x)
    if op in ("wt2", "wt4"):
        return dict(w=_weight(c["kind"], c["Cout"], c["Cin"], g))
    if op in ("out2", "out4", "chain2", "chain4"):
        B, H, W, C = c["B"], c["H"], c["W"], c["C"]
        P = B * (H // m) * (W // m)
        d["Y"] = _fill(c["kind"], ((m + 2) ** 2, P, C), g) * (1.0 if m == 2 else 2.0 ** -5)      # (F(4x4): |A^T| 1 |A| = 324, the operand holds 16 376)
        if c["bias"]:
            d["bias"] = torch.randn(C, generator=g)
        for i in range(c.get("nres", 0)):
            d[f"r{i + 1}"] = torch.randn(B, H, W, C, generator=g)
        return d
    if op == "narrow":
        x = _fill(c["kind"], (c["B"], c["H"], c["W"], c["C"]), g)
        d = dict(x=quantise(x) if c["hl"] else x, w=torch.randn(c["Cout"], c["C"], c["k"], c["k"], generator=g) / (c["C"] * c["k"] ** 2) ** 0.5,
                 bias=torch.randn(c["Cout"], generator=g))
        if c["res"]:
            d["r1"] = torch.randn(c["B"], c["H"], c["W"], c["Cout"], generator=g)
        return d
    # conv_w2 / conv_w4 / pair4
    B, H, W, Ci = c["B"], c["H"], c["W"], c["Cin"]
    x = _image(c["kind"], B, H, W, Ci, m, g)
    d["x"] = quantise(x) if fam == 4 else x
    wk = c["kind"] if c["kind"] in ("impulse", "decades") else "randn"
    couts = (c["Ca"], c["Cb"]) if op == "pair4" else (c["Cout"],)
    for n, co in zip(("w", "wb"), couts):
        d[n] = _weight(wk, co, Ci, g)
        if c["bias"]:
            d["bias" if n == "w" else "biasb"] = torch.randn(co, generator=g)
    for i in range(c.get("nres", 0)):
        d[f"r{i + 1}"] = torch.randn(B, H, W, couts[0], generator=g)
    return d


# ------------------------------------------------------------------------------------------------------------------ tiles and layouts
def _tiles(x, m, wrong=None):
    """x (B, H, W, C) -> (P, t, t, C): the (m + 2)^2 window of every tile, zero outside the image"""
    B, H, W, C = x.shape
    t, th, tw = m + 2, H // m, W // m
    r = torch.arange(th * tw)
    ty, tx = (r // th, r % th) if wrong == "thtw_swapped" else (r // tw, r % tw)
    k = torch.arange(t)
    iy, ix = (m * ty - 1).view(-1, 1) + k, (m * tx - 1).view(-1, 1) + k
    if wrong == "ring_slot":                                # the halo row below, read from the slot of the tile row itself
        iy[:, t - 1] = torch.where(iy[:, t - 1] < H, m * ty, iy[:, t - 1])
    ok = ((iy >= 0) & (iy < H))[:, :, None] & ((ix >= 0) & (ix < W))[:, None, :]
    g = x[:, iy.clamp(0, H - 1)[:, :, None], ix.clamp(0, W - 1)[:, None, :], :]              # (B, T, t, t, C)
    if wrong != "pad_clamp":
        g = g * ok[None, :, :, :, None].to(x.dtype)
    return g.reshape(B * th * tw, t, t, C)


def _place(o, B, H, W, m):
    """(P, m, m, C) -> (B, H, W, C)"""
    return o.reshape(B, H // m, W // m, m, m, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, -1)


def _in_mat(x, m, relu, absolute=False):
    d = _tiles(F.relu(x) if relu else x, m)
    M = BT[m].abs() if absolute else BT[m]
    u = torch.einsum("ai,pijc,bj->abpc", M, d.abs() if absolute else d, M)
    return u.reshape((m + 2) ** 2, -1, x.shape[-1])


def _wt_mat(w, m, absolute=False):
    M = G[m].abs() if absolute else G[m]
    v = torch.einsum("ak,ockl,bl->aboc", M, w.abs() if absolute else w, M)
    return v.reshape((m + 2) ** 2, w.shape[0], w.shape[1])


def _out_mat(Y, m, B, H, W, absolute=False):
    t = m + 2
    M = AT[m].abs() if absolute else AT[m]
    o = torch.einsum("ia,abpc,jb->pijc", M, (Y.abs() if absolute else Y).reshape(t, t, Y.shape[1], Y.shape[2]), M)
    return _place(o, B, H, W, m)


# ------------------------------------------------------------------------------------------------------------------ the kernels' order
def _along(f, X, d):
    return torch.stack(f(list(X.unbind(d))), d)


def _bt2(d):
    return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]


def _bt4(d, five=5.0):
    a_, b_, c_, e_ = d[4] - 4.0 * d[2], d[3] - 4.0 * d[1], d[4] - d[2], 2.0 * (d[3] - d[1])
    return [4.0 * d[0] - five * d[2] + d[4], a_ + b_, a_ - b_, c_ + e_, c_ - e_, 4.0 * d[1] - 5.0 * d[3] + d[5]]


def _g2(g):
    return [g[0], 0.5 * (g[0] + g[1] + g[2]), 0.5 * (g[0] - g[1] + g[2]), g[2]]


def _g6(g):
    # (a python scalar times an fp32 tensor: the constant is rounded to fp32 once, then the product)
    return [0.25 * g[0], (-1.0 / 6.0) * ((g[0] + g[2]) + g[1]), (-1.0 / 6.0) * ((g[0] + g[2]) - g[1]),
            (1.0 / 24.0) * g[0] + (1.0 / 12.0) * g[1] + (1.0 / 6.0) * g[2], (1.0 / 24.0) * g[0] - (1.0 / 12.0) * g[1] + (1.0 / 6.0) * g[2], g[2]]


def _at2(y):
    return [(y[0] + y[1]) + y[2], (y[1] - y[2]) - y[3]]


def _at4(y, eight=8.0):
    s12, d12, s34, d34 = y[1] + y[2], y[1] - y[2], y[3] + y[4], y[3] - y[4]
    return [(y[0] + s12) + s34, d12 + 2.0 * d34, s12 + 4.0 * s34, (d12 + eight * d34) + y[5]]


def _split(a, lo=True):
    """(hi, lo) fp16 terms of a (already in operand scale) as values in a's dtype; beyond the fp16 range hi is +-inf, as wino_split4's"""
    hi = a.half().to(a.dtype)
    return hi, ((a - hi).half().to(a.dtype) if lo else torch.zeros_like(a))


def _in_impl(x, m, relu, wrong=None):
    """U (t^2, P, C) in x's dtype; F(4x4): the (hi, lo) terms of U / 16 from the operand's values x"""
    d = _tiles(x * 4.0 if m == 4 else x, m, wrong if wrong in ("thtw_swapped", "pad_clamp", "ring_slot") else None)
    if relu:
        d = d.clamp_min(0.0)
    bt = _bt2 if m == 2 else ((lambda v: _bt4(v, 4.0)) if wrong == "bt_coeff" else _bt4)
    u = _along(bt, _along(bt, d, 1), 2).permute(1, 2, 0, 3).reshape((m + 2) ** 2, d.shape[0], d.shape[3])
    if m == 2:
        return u
    return _split(u * (1.0 / 64.0), lo=wrong != "lo_dropped")


def _wt_impl(w, m):
    g = _g2 if m == 2 else _g6
    v = _along(g, _along(g, w, 2), 3).permute(2, 3, 0, 1)
    return v.reshape((m + 2) ** 2, w.shape[0], w.shape[1])


def _act(v, act):
    if act == "relu":
        return v.clamp_min(0.0)
    if act == "leaky01":
        return torch.maximum(v, v * 0.1)
    return v


def _epi_impl(v, c, t, wrong=None):
    """bias, activation, residuals, operand rounding on the placed map v, in v's dtype"""
    if "bias" in t:
        v = v + t["bias"]
    v = _act(v, c.get("act"))
    for k in ("r1", "r2"):
        if k in t:
            v = v + t[k]
    if c.get("hl") or c.get("also"):
        relu = (c.get("c_relu") or c.get("also") == "relu") and wrong != "c_relu_ignored"
        a = v * 4.0
        hi, lo = _split(a.clamp_min(0.0) if relu else a)
        h = (hi + lo) / 4.0
        return (v, h) if c.get("also") else h
    return v


def _out_impl(Y, m, c, t, wrong=None):
    tt = m + 2
    at = _at2 if m == 2 else ((lambda v: _at4(v, 4.0)) if wrong == "at_coeff" else _at4)
    o = _along(at, _along(at, Y.reshape(tt, tt, Y.shape[1], Y.shape[2]), 0), 1).permute(2, 0, 1, 3)
    return _epi_impl(_place(o, c["B"], c["H"], c["W"], m), c, t, wrong)


def _products(Uo, V, m, dtype):
    """Y (t^2, P, Cout) in the engine's arithmetic: fp32 products and sums (F(2x2)); F(4x4): hi hi + hi lo + lo hi of the operands, the weight
    operand at its power-of-two scale (engine_bounds.weight_exponent), fp32 accumulation, x 16 for the scale of U"""
    def e(a, b):      # one multiply and one add per channel, ascending: element-wise torch ops, the same bits on every host
        acc = torch.zeros(a.shape[0], a.shape[1], b.shape[1], dtype=a.dtype)
        for ch in range(a.shape[2]):
            acc = acc + a[:, :, None, ch] * b[:, None, :, ch]
        return acc

    if m == 2:
        return e(Uo, V)
    (uh, ul), s = Uo, 2.0 ** eb.weight_exponent(V)
    vh, vl = _split(V * s)
    return (e(uh, vh) + e(uh, vl) + e(ul, vh)) * (16.0 / s)


def _narrow_impl(t, c):
    """the sequential multiply-add chain of conv_narrow_kernel: 32-channel slices, taps row-major, channels ascending"""
    x, w = t["x"], t["w"]
    B, H, W, C = x.shape
    k, r = c["k"], c["k"] // 2
    xp = F.pad(x.permute(0, 3, 1, 2), (r, r, r, r)).permute(0, 2, 3, 1)
    acc = torch.zeros(B, H, W, c["Cout"], dtype=x.dtype)
    for c0 in range(0, C, 32):
        for dy in range(k):
            for dx in range(k):
                for ch in range(c0, c0 + 32):
                    acc = acc + xp[:, dy:dy + H, dx:dx + W, ch, None] * w[:, ch, dy, dx]
    v = acc + t["bias"]
    return v + t["r1"] if "r1" in t else v


def impl(op, c, inp, dtype=torch.float32, wrong=None):
    t = {k: v.to(dtype) for k, v in inp.items()}
    m = fam_of(op) if op != "narrow" else 4
    if op in ("in2", "in4"):
        u = _in_impl(t["x"], m, c["relu"], wrong)
        return u if m == 2 else (u[0] + u[1]) * 16.0
    if op in ("wt2", "wt4"):
        return _wt_impl(t["w"], m)
    if op in ("out2", "out4"):
        return _out_impl(t["Y"], m, c, t, wrong)
    if op in ("chain2", "chain4"):
        # h = act(A^T Y A + bias), the consumer's ReLU folded in; F(4x4): rounded to the operand's 22 bits as the operand store would
        h = _out_impl(t["Y"], m, dict(c, hl=(m == 4)), t, wrong)
        if m == 2 and c["c_relu"] and wrong != "c_relu_ignored":
            h = h.clamp_min(0.0)
        u = _in_impl(h, m, False, wrong)
        return u if m == 2 else (u[0] + u[1]) * 16.0
    if op == "narrow":
        return _narrow_impl(t, c)
    outs = []
    Uo = _in_impl(t["x"], m, c["relu_in"], wrong)
    ws = [t["w"]] + ([t["wb"]] if op == "pair4" else [])
    V = torch.cat([_wt_impl(w, m) for w in ws], 1)                                            # the pair: one product over the concatenated filters
    Y = _products(Uo, V, m, dtype)
    col = 0
    for i, w in enumerate(ws):
        co = w.shape[0]
        sl = Y[:, :, 0:co] if (wrong == "pair_col0" and i == 1) else Y[:, :, col:col + co]
        te = {k: v for k, v in t.items() if k in ("r1", "r2")}
        if ("bias", "biasb")[i] in t:
            te["bias"] = t[("bias", "biasb")[i]]
        outs.append(_out_impl(sl, m, c, te, wrong))
        col += co
    return tuple(outs) if op == "pair4" else outs[0]


# ------------------------------------------------------------------------------------------------------------------ the models
def _in_model(x, m, relu):
    ref, A = _in_mat(x, m, relu), _in_mat(x, m, relu, absolute=True)
    mod = K_IN[m] * U * A
    if m == 4:
        mod = torch.where(A > 0, mod + SPLIT_REL * ref.abs() + FLOOR_U, torch.zeros_like(A))
    return ref, mod


def _epi_model(pre, bpre, c, d):
    """(ref, epilogue model) of bias, activation, residuals and the operand rounding after a pre-activation `pre` known to `bpre` (which
    passes the activation with Lipschitz constant 1 and is not part of the result); two results with `also`"""
    b = torch.zeros_like(pre)
    if "bias" in d:
        pre, b = pre + d["bias"], b + eb.EPI * d["bias"].abs()
    y = eb.ACT_F[c.get("act")](pre)
    b = b + eb.EPI * y.abs()
    for k in ("r1", "r2"):
        if k in d:
            y = y + d[k]
            b = b + eb.EPI * d[k].abs() + U * y.abs()
    if c.get("hl") or c.get("also"):
        h = F.relu(y) if (c.get("c_relu") or c.get("also") == "relu") else y
        bh = b + torch.where((b + (0 if bpre is None else bpre) > 0) | (h != 0), SPLIT_REL * h.abs() + eb.FLOOR_ACT, torch.zeros_like(b))
        return ((y, h), (b, bh)) if c.get("also") else (h, bh)
    return y, b


def model(op, c, inp):
    """(ref, model, fixed): bound = MARGIN x model + fixed.  `fixed` is the part that already carries the margin of the stage it belongs to
    and takes no other: the epilogue terms of the end-to-end ops and of narrow (out2's / out4's margin: the same fp32 adds and the same
    operand split), the hidden map's bound carried through the input transform of a chain; zero for the stage ops"""
    d = {k: v.double() for k, v in inp.items()}
    m = fam_of(op) if op != "narrow" else 4
    if op in ("in2", "in4"):
        ref, mod = _in_model(d["x"], m, c["relu"])
        return ref, mod, torch.zeros_like(mod)
    if op in ("wt2", "wt4"):
        mod = K_W[m] * U * _wt_mat(d["w"], m, absolute=True)
        return _wt_mat(d["w"], m), mod, torch.zeros_like(mod)
    B, H, W = c["B"], c["H"], c["W"]
    if op in ("out2", "out4"):
        bpre = K_OUT[m] * U * _out_mat(d["Y"], m, B, H, W, absolute=True)
        y, b = _epi_model(_out_mat(d["Y"], m, B, H, W), bpre, c, d)
        mod = bpre + b
        return y, mod, torch.zeros_like(mod)
    if op in ("chain2", "chain4"):
        bpre = K_OUT[m] * U * _out_mat(d["Y"], m, B, H, W, absolute=True)
        h, b = _epi_model(_out_mat(d["Y"], m, B, H, W), bpre, dict(c, hl=(m == 4)), d)
        bh = (bpre + b) * MARGIN[f"out{m}"]
        if m == 2 and c["c_relu"]:
            h = F.relu(h)
        ref, mod = _in_model(h, m, False)
        carried = _in_mat(bh, m, False, absolute=True)
        if m == 4:      # (a hidden value known to bh: the split of U sees it as well, and may turn a zero window into a non-zero one)
            carried = torch.where(carried > 0, carried * (1 + SPLIT_REL) + MARGIN["in4"] * FLOOR_U * (mod == 0), carried)
        return ref, mod, carried
    if op == "narrow":
        xn = d["x"].permute(0, 3, 1, 2)
        pre, bpre = eb.reference("conv2d", xn, d["w"], "f32", device="cpu", padding=c["k"] // 2)
        de = dict(bias=d["bias"], **({"r1": d["r1"]} if "r1" in d else {}))
        y, b = _epi_model(pre.permute(0, 2, 3, 1), None, {}, de)
        return y, bpre.permute(0, 2, 3, 1), MARGIN["out2"] * b
    # end to end
    x = F.relu(d["x"]) if c["relu_in"] else d["x"]
    ws = [d["w"]] + ([d["wb"]] if op == "pair4" else [])
    Ua = _in_mat(x, m, False, absolute=True)
    Vall = torch.cat([_wt_mat(w, m) for w in ws], 1)
    k = K_IN[m] + K_W[m] + K_OUT[m]
    outs = []
    for i, w in enumerate(ws):
        pre = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
        Va = _wt_mat(w, m, absolute=True)
        e = lambda a, b: torch.einsum("xpc,xoc->xpo", a, b)   # noqa: E731
        Yb = (k * U + eb.TAU["f32" if m == 2 else "f16x3"]) * e(Ua, Va)
        if m == 4:
            Yb = Yb + FLOOR_U * e((Ua > 0).double(), Va) + eb.floor_w(Vall) * e(Ua, torch.ones_like(Va))
        de = {kk: v for kk, v in d.items() if kk in ("r1", "r2")}
        if ("bias", "biasb")[i] in d:
            de["bias"] = d[("bias", "biasb")[i]]
        bpre = _out_mat(Yb, m, B, H, W, absolute=True)
        y, b = _epi_model(pre, bpre, c, de)
        if c.get("also"):
            outs += [(y[0], bpre, MARGIN[f"out{m}"] * b[0]), (y[1], bpre, MARGIN[f"out{m}"] * b[1])]
        else:
            outs.append((y, bpre, MARGIN[f"out{m}"] * b))
    if len(outs) > 1:
        return tuple(o[0] for o in outs), tuple(o[1] for o in outs), tuple(o[2] for o in outs)
    return outs[0]


MARGIN_OF = {"chain2": "in2", "chain4": "in4", "pair4": "conv_w4"}     # ops without a margin of their own: composed from the stages'


def reference(op, c, inp):
    """(ref, bound) = (the float64 result, MARGIN x model + fixed); tuples where the op has two results"""
    ref, mod, fixed = model(op, c, inp)
    k = MARGIN[MARGIN_OF.get(op, op)]
    if isinstance(mod, tuple):
        return ref, tuple(k * a + b for a, b in zip(mod, fixed))
    return ref, k * mod + fixed


def excess_ratio(got, ref, mod, fixed):
    """worst (|got - ref| - fixed)+ / model over all outputs (0 / 0 counts as 0)"""
    if not isinstance(ref, tuple):
        got, ref, mod, fixed = (got,), (ref,), (mod,), (fixed,)
    return max(worst_ratio(r + ((a.detach().double() - r).abs() - f).clamp_min(0), r, b) for a, r, b, f in zip(got, ref, mod, fixed))


CASES = _cases()
OPS = list(CASES)
NONSQUARE = lambda c: c["H"] != c["W"]   # noqa: E731
# wrong variant -> the rule under which a case contains its error
WRONG = {
    "in2": {"thtw_swapped": NONSQUARE, "pad_clamp": lambda c: c["kind"] not in ("sparse", "impulse", "dead")},
    "in4": {"thtw_swapped": NONSQUARE, "pad_clamp": lambda c: c["kind"] not in ("sparse", "impulse", "dead"),
            "bt_coeff": lambda c: c["kind"] != "dead", "lo_dropped": lambda c: c["kind"] in ("randn", "decades", "offset")},
    "out4": {"at_coeff": lambda c: True, "c_relu_ignored": lambda c: bool(c.get("hl") and c.get("c_relu"))},
    "chain2": {"ring_slot": lambda c: c["H"] > 2, "c_relu_ignored": lambda c: c["c_relu"] and c["act"] != "relu"},
    "chain4": {"ring_slot": lambda c: c["H"] > 4, "c_relu_ignored": lambda c: c["c_relu"] and c["act"] != "relu"},
    "conv_w2": {"thtw_swapped": NONSQUARE, "pad_clamp": lambda c: c["kind"] not in ("sparse", "dead")},
    "conv_w4": {"thtw_swapped": NONSQUARE, "bt_coeff": lambda c: c["kind"] != "dead", "at_coeff": lambda c: c["kind"] != "dead",
                "lo_dropped": lambda c: c["kind"] in ("randn", "decades", "offset")},
    "pair4": {"pair_col0": lambda c: True},
}
# variants that can show on non-square maps only: the CPU test asserts that they stay inside the bound on every square case
ONLY_NONSQUARE = ("thtw_swapped",)
