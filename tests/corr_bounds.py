"""Float64 references and element-wise error bounds for the correlation pyramid + lookup (csrc/pp_corr.hip) and its adjoint
(corr_lookup_backward_kernel / corr_lookup_scatter_kernel in csrc/pp_backward3.hip).  A helper of tests/test_corr_bounds_{cpu,gpu}.py,
imported through sys.path like tests/kernel_bounds.py, whose sampling model, cs(), _bilinear / _slopes and _upstream it reuses.  The loss
kernels (gather + normalise, diagonal cross entropy, flow / certainty loss, ordered row scatter) follow in the second half of the file,
with their models above their code.

    inputs(op, case)                        fp32 CPU tensors
    reference(op, case, inp) -> (ref, bound)  float64 CPU tensors (tuples for the adjoint: df1, df2, dflow)
    impl(op, case, inp, dtype, wrong=None)  the kernels' formula restated in torch in `dtype`: float32 sets the margins, float64 + wrong is a
                                            structurally wrong variant

ref comes from torch's own float64 ops only: the MATERIALISED volume corr = einsum(f1, f2) / sqrt(C), pooled with F.avg_pool2d (the volume is
pooled, as the reference project does, not f2), sampled with F.grid_sample(align_corners=True, padding_mode="zeros") at (p + flow) / 2^l +
delta after the round trip x * 2 / max(size - 1, 1) - 1, channel l win^2 + a win + b = x offset a - r, y offset b - r; the adjoint is
float64 autograd of exactly that.  Never oracle/, impl() or this project's kernels.  Two conventions are the kernels' documented ones, not
torch's: a pixel whose flow has a NaN or infinite component is an out-of-image sample (ref and every gradient of that pixel exactly 0; the
reference is evaluated with the flow replaced by 0 there and masked), and nothing else.  On a pooled axis of size 1 torch's own
de-normalisation multiplies by size - 1 = 0: every offset samples coordinate 0 and the flow gradient along that axis is exactly 0.

impl restates the kernels: f2 pooled ((a + b) + (c + d)) / 4 per level rather than the volume, the (2r+2)^2 table of dot products around
the CENTRE's round trip, clamped to [-(r+2), size + r + 1] (NaN -> the lower clamp), integer offsets, the four-corner blend
t00 (wx0 wy0) + t01 (wx1 wy0) + t10 (wx0 wy1) + t11 (wx1 wy1) with wx0 = 1 - wx1; a sequential fma chain is approximated by a torch dot in
`dtype`.  Operand modes: hi = f16(4x), lo = f16(4x - hi), product hi hi + hi lo + lo hi (f16x3) or hi hi alone (f16), as engine_bounds
describes; the pooled levels are split after pooling.  The adjoint of impl is torch autograd of that formula in `dtype` (clamp and floor pass
no gradient: the kernels' rx == cx rule).

Models, u = 2^-24, tw = 2r + 2, win = 2r + 1, A_l[p, q] = sum_c |f1[p, c]| pool_l(|f2|)[q, c] / sqrt(C):
* corr, a table value: tb = (TAU[mode] + (3 l + 1) u) A_l + FLOOR_ACT (sum_c |f1[p]| + pool_l(sum_c |f2|)[q]) / sqrt(C) in the operand modes (no
  floors in f32): the engine's contraction model, 3 l u for l poolings (kernel_bounds' avgpool2 model, relative to pool(|f2|)), 1 u for the scaling.
  A sample: sum_t w_t tb_t + 7 u S + slope_x dix + slope_y diy, S = sum_t w_t |T_t| and the slopes those of the zero-padded float64 table
  T_l[p, .] (kb._slopes on the volume viewed as B HW one-channel images), dix = 4 u max(|ix|, Wl - 1) (the round trip of (x + flow) / 2^l;
  the division by 2^l is exact), 0 on an axis of size 1; plus the second-order term dix diy max(|t00| + |t01| + |t10| + |t11|) over the cells the
  coordinate box touches (both slopes vanish where both coordinates sit on an integer whose other row and column are outside).
  Samples whose four taps are outside for every coordinate in the box: model 0.  Pad channels: exactly 0 (GPU test).
* corr_bwd.  W_l = the adjoint weights sum |dout| w (every corner product rounds, the 4-term fma chain of dt: the 8 below).
  df1[p, c] = sum_l sum_q dt f2_l[q, c] / sqrt(C): (cs(tw^2 L) + 8 + 3 l) u sum W_l pool_l(|f2|) / sqrt(C) + the coordinate term: the same sum
  with the weights' sensitivities dix |dw/dx| + diy |dw/dy| in place of w.
  df2 (after the pooling chain's adjoint): (m + 4 + 8) u sum |contribution| + coordinate term, contributions |W_l| |f1| / sqrt(C) carried down the
  pooling adjoint (x 0.25 per level, exact), m = the number of (pixel, table position) pairs that reach the element through the chain, + L.
  Deterministic (2^-40 fixed point): (min(m, 16) + 8 + L) u sum |contribution| + m 2^-41 + u |v| (a patch entry is a 16-term fp32 sum; the
  integer sum itself is exact), bit-identical over two runs.
  dflow_x = sum_l (1 / 2^l) sum_out dout (T01 - T00) wy0 + (T11 - T10) wy1:  u (cs(C) + 8 + 3 l) sum |dout| (wy0 (A00 + A01) + wy1 (A10 + A11)) / 2^l
  + diy sum |dout| |(T01 - T00) - (T11 - T10)| / 2^l.  Where a level's coordinate lies within 1e-4 of an integer (axis longer than 1, inside the
  clamp) the one-sided derivatives differ: that component is held to sum |left - right| + bound, summed over the levels and the window
  offsets along that axis, left / right = the float64 reference gradient of that group of samples with that flow component moved by
  -/+ 1e-3 (in fp32 every level falls to its own side, and the reference round-trips every offset on its own), and the df1 / dflow models
  of such a pixel are the largest of the four cells around the coordinate, its df2 contributions those of all four.  A clamped coordinate has every tap outside (A = 0: model 0); an axis of pooled size 1 contributes exactly 0.

Margins: MARGIN[op] <= 4 x the worst |impl_fp32 - ref| / model over the sweep, measured on the CPU by tests/test_corr_bounds_cpu.py, never from
the HIP kernels; one margin per arithmetic mode for corr.  They are set at about 3 x the measured value: torch's fp32 sums depend on the host's
thread count and vector width (the measured worst ratio moved by up to 20 % between two hosts), and the CPU test holds it to
[margin / 4, margin] on whichever host it runs.
"""
import math

import torch
import torch.nn.functional as F

import engine_bounds as eb
import kernel_bounds as kb

U = kb.U
cs = kb.cs
check = eb.check
MEASURED, MARGIN = {}, {}


def _set(op, measured, margin):
    assert margin <= 4.0 * measured + 1e-12, (op, measured, margin)
    MEASURED[op], MARGIN[op] = measured, margin


_set("corr:f32", 0.521, 1.6)
_set("corr:f16x3", 0.519, 1.6)
_set("corr:f16", 0.668, 2.0)
_set("corr_bwd", 0.214, 0.65)
_set("corr_bwd_det", 0.214, 0.65)

MODES = ("f32", "f16x3", "f16")
FLOWS = ("smooth", "noisy", "plus_border", "minus_border", "far", "integer", "nonfinite", "half")
# kinds whose near-integer coordinates are planted (accounted apart from the 1 % cap): the two border kinds are uniform INTEGER flows
PLANTED = ("integer", "half", "plus_border", "minus_border")

# (H, W, levels, r, C): the lane-per-position path, then the tiled path (H, W % 8 == 0, C % 32 == 0)
LANE = [(5, 7, 1, 2, 4), (6, 10, 2, 1, 12), (12, 20, 3, 2, 36), (4, 8, 3, 2, 8), (8, 4, 3, 1, 8)]
TILED = [(8, 8, 1, 2, 32), (8, 8, 3, 1, 32), (16, 32, 2, 2, 64), (24, 40, 3, 2, 64), (32, 32, 3, 2, 256)]
# the adjoint's patch kernel (H, W % 4 == 0, C % 128 == 0); the last two: a pooled axis of size 1 ON that kernel (one patch row / column)
PATCH = [(8, 8, 3, 2, 128), (16, 16, 3, 2, 256), (4, 8, 3, 2, 128), (8, 4, 3, 1, 128)]


def _cases():
    fwd, bwd = [], []
    for i, (H, W, L, r, C) in enumerate(LANE + TILED):
        small = (H, W) in ((5, 7), (8, 8), (4, 8), (8, 4))
        kinds = FLOWS if small else [FLOWS[(3 * i + k) % len(FLOWS)] for k in range(3)]
        for j, kind in enumerate(kinds):
            fwd.append(dict(H=H, W=W, L=L, r=r, C=C, B=3, fb=(1, 3)[(i + j) % 2], ld_flow=(2, 4)[j % 2], kind=kind))
    fwd.append(dict(H=6, W=10, L=2, r=1, C=12, B=4, fb=2, ld_flow=2, kind="noisy"))      # (b % f2_batch differs from b f2_batch // B)
    for i, (H, W, L, r, C) in enumerate(LANE + TILED[:4] + PATCH + TILED[4:]):
        small = H * W <= 64
        kinds = ("noisy", "nonfinite", "integer", "half", "plus_border") if small else [("noisy", "smooth", "minus_border")[i % 3]]
        for j, kind in enumerate(kinds):
            bwd.append(dict(H=H, W=W, L=L, r=r, C=C, B=1 if H * W * C > 60000 else 2, ld_flow=(2, 4)[(i + j) % 2], kind=kind))
    return dict(corr=fwd, corr_bwd=bwd)


_CORR_CASES = _cases()


def case_name(op, c):
    return op + "(" + ",".join(f"{k}={v}" for k, v in c.items()) + ")"


def flat_axes(c):
    """(x, y): the levels' pooled width / height reaches 1"""
    return (c["W"] >> (c["L"] - 1)) == 1, (c["H"] >> (c["L"] - 1)) == 1


def make_flow(kind, B, H, W, ld, g):
    """the flow kinds of tests/test_corr_lookup_ring_gpu.py, plus `nonfinite` (1 % of the pixels NaN / +inf / -inf in either component) and `half`
    (x.5 targets: both weights 0.5 at level 0)"""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    # (that file's smooth field 0.15 x - 0.1 y + 1.3, 0.1 x + 0.2 y - 2.1 with its coefficients moved off the decimal grid: there 7 % of the targets
    # are integers at some level, which the adjoint's cap on near-integer coordinates does not admit)
    smooth = torch.stack([0.1513 * xx - 0.1007 * yy + 1.3071, 0.1009 * xx + 0.2011 * yy - 2.1037], dim=-1)[None].repeat(B, 1, 1, 1)
    if kind == "smooth":
        fl = smooth
    elif kind in ("noisy", "nonfinite"):
        fl = smooth + 3.0 * torch.randn(B, H, W, 2, generator=g)
    elif kind in ("plus_border", "minus_border"):
        fl = smooth * 0.0 + (1.0 if kind == "plus_border" else -1.0) * torch.tensor([W - 2.0, H - 2.0])
    elif kind == "far":
        fl = smooth * 0.0 + 1.0e4
    elif kind == "integer":
        fl = torch.randint(-3, 4, (B, H, W, 2), generator=g).float()
    else:
        fl = torch.randint(-3, 3, (B, H, W, 2), generator=g).float() + 0.5
    out = torch.randn(B, H, W, ld, generator=g)
    out[..., :2] = fl
    if kind == "nonfinite":
        n = max(3, B * H * W // 100)
        idx = torch.randperm(B * H * W, generator=g)[:n]
        v = out.view(-1, ld)
        for k, i in enumerate(idx.tolist()):
            v[i, k % 2] = (float("nan"), float("inf"), float("-inf"))[k % 3]
    return out


def _corr_inputs(op, c, seed=0):
    g = kb._gen(7000 * ("corr", "corr_bwd").index(op) + seed + sum(int(v) * 7 if isinstance(v, int) else len(v) for v in c.values()))
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    fb = c.get("fb", B)
    f1 = torch.randn(B, H, W, C, generator=g) * kb._row_scales(g, B, 1.0).view(-1, 1, 1, 1)
    f2 = torch.randn(fb, H, W, C, generator=g) * kb._row_scales(g, fb, 1.0).view(-1, 1, 1, 1)
    d = dict(f1=f1, f2=f2, flow=make_flow(c["kind"], B, H, W, c["ld_flow"], g))
    if op == "corr_bwd":
        d["dout"] = kb._upstream(g, (B, H, W, c["L"] * (2 * c["r"] + 1) ** 2))
    return d


# ------------------------------------------------------------------------------------------------------------------ the float64 reference
def _bad(flow):
    return ~torch.isfinite(flow[..., :2]).all(-1)


def _grid_px(flow):
    H, W = flow.shape[1:3]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=flow.dtype), torch.arange(W, dtype=flow.dtype), indexing="ij")
    return xs + flow[..., 0], ys + flow[..., 1]


def ref_forward(f1, f2, flow, L, r):
    """the materialised pyramid + grid_sample, float64, differentiable; f2 already expanded to f1's batch"""
    B, H, W, C = f1.shape
    win = 2 * r + 1
    bad = _bad(flow)
    fl = torch.where(bad.unsqueeze(-1), torch.zeros((), dtype=flow.dtype), flow[..., :2])
    vol = torch.einsum("bpc,bqc->bpq", f1.reshape(B, H * W, C), f2.reshape(B, H * W, C)) / math.sqrt(C)
    vol = vol.reshape(B * H * W, 1, H, W)
    px, py = _grid_px(fl)
    px, py = px.reshape(-1, 1), py.reshape(-1, 1)
    d = torch.arange(-r, r + 1, dtype=f1.dtype).view(1, -1)
    outs, vols = [], []
    for l in range(L):
        if l:
            vol = F.avg_pool2d(vol, 2)
        Hl, Wl = vol.shape[-2:]
        gx = (px / 2 ** l + d) * 2 / max(Wl - 1, 1) - 1
        gy = (py / 2 ** l + d) * 2 / max(Hl - 1, 1) - 1
        grid = torch.stack([gx[:, :, None].expand(-1, win, win), gy[:, None, :].expand(-1, win, win)], -1)      # [n, a, b] = (x of a, y of b)
        s = F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        outs.append(s.reshape(B, H, W, win * win))
        vols.append(vol)
    out = torch.cat(outs, -1)
    return torch.where(bad.unsqueeze(-1), torch.zeros((), dtype=out.dtype), out), vols


# ------------------------------------------------------------------------------------------------------ the kernels' formula in torch
def _level_coords(flow, H, W, l, r, wrong=None):
    """(cx, cy) of level l as the kernels compute them, in flow's dtype: the centre's round trip, clamped (NaN -> the lower clamp)"""
    gx, gy = _grid_px(flow)
    Hl, Wl = H >> l, W >> l

    def one(g, size):
        if wrong == "level_coord_half":
            c = g
            for _ in range(l):
                c = (c + 0.5) / 2 - 0.5
        else:
            c = g / 2 ** l
        n = c * 2 / max(size - 1, 1) - 1
        rt = ((n + 1) / 2) * (size - 1)
        if wrong in ("dflow_no_level_scale", "flat_axis_gradient"):      # the value as computed, the derivative of another formula
            if wrong == "dflow_no_level_scale":
                rt = rt.detach() + (g - g.detach())
            elif size == 1:
                rt = rt.detach() + (c - c.detach())
        lo, hi = -(r + 2.0), size + r + 1.0
        return torch.where(torch.isnan(rt), torch.full_like(rt, lo), rt).clamp(lo, hi)

    return one(gx, Wl), one(gy, Hl)


def _split(x, mode):
    """the operand terms of x at scale 4 as fp32-exact values in x's dtype: [(hi, lo)] f16x3, [(hi, 0)] f16"""
    a = x.float() * 4
    hi = a.half().float()
    lo = (a - hi).half().float()
    return (hi.to(x.dtype) / 4, (lo.to(x.dtype) / 4) if mode == "f16x3" else None)


def _dot(f1n, G, mode):
    """<f1[n], G[n, y, x]> over channels in the arithmetic of `mode`"""
    e = lambda a, b: torch.einsum("nc,nyxc->nyx", a, b)   # noqa: E731
    if mode == "f32":
        return e(f1n, G)
    (h1, l1), (h2, l2) = _split(f1n, mode), _split(G, mode)
    if mode == "f16":
        return e(h1, h2)
    return e(h1, h2) + e(h1, l2) + e(l1, h2)


def _pool(x):
    a, b, c, d = x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]
    Ho, Wo = x.shape[1] // 2, x.shape[2] // 2
    return ((a[:, :Ho, :Wo] + b[:, :Ho, :Wo]) + (c[:, :Ho, :Wo] + d[:, :Ho, :Wo])) * 0.25


def _table(f1n, f2l, bidx, cx, cy, r, mode, pad="zeros"):
    """tab[n, dy, dx] = <f1[n], f2l[b(n), by + dy, bx + dx]> (0 outside), and the inside mask with the clamped positions"""
    tw = 2 * r + 2
    Hl, Wl = f2l.shape[1:3]
    k = torch.arange(tw)
    qx = (torch.floor(cx).long() - r).view(-1, 1) + k
    qy = (torch.floor(cy).long() - r).view(-1, 1) + k
    inside = ((qy >= 0) & (qy < Hl))[:, :, None] & ((qx >= 0) & (qx < Wl))[:, None, :]
    qxc, qyc = qx.clamp(0, Wl - 1), qy.clamp(0, Hl - 1)
    G = f2l[bidx.view(-1, 1, 1), qyc[:, :, None], qxc[:, None, :]]
    tab = _dot(f1n, G, mode)
    if pad == "zeros":
        tab = torch.where(inside, tab, torch.zeros((), dtype=tab.dtype))
    return tab, inside, qyc, qxc


def _corners(tab, r, flat_x, flat_y, wrong=None):
    """(t00, t01, t10, t11) as [n, a, b]: the table entries the sample of x offset a - r, y offset b - r blends"""
    win = 2 * r + 1
    ai = torch.full((win,), r) if flat_x and wrong != "flat_axis_as_today" else torch.arange(win)
    bi = torch.full((win,), r) if flat_y and wrong != "flat_axis_as_today" else torch.arange(win)
    pick = lambda dy, dx: tab[:, (bi + dy)][:, :, (ai + dx)].transpose(1, 2)   # noqa: E731
    return pick(0, 0), pick(0, 1), pick(1, 0), pick(1, 1)


def _blend(tab, cx, cy, r, flat_x, flat_y, wrong=None):
    t00, t01, t10, t11 = _corners(tab, r, flat_x, flat_y, wrong)
    wx1, wy1 = (cx - torch.floor(cx)).view(-1, 1, 1), (cy - torch.floor(cy)).view(-1, 1, 1)
    wx0, wy0 = 1 - wx1, 1 - wy1
    out = t00 * (wx0 * wy0) + t01 * (wx1 * wy0) + t10 * (wx0 * wy1)
    if wrong != "df2_missing_corner":
        out = out + t11 * (wx1 * wy1)
    if wrong == "window_transposed":
        out = out.transpose(1, 2)
    return out


def _lookup(f1, f2, flow, c, mode="f32", wrong=None):
    """the lookup as the kernels compute it, in f1's dtype, differentiable: (B, H, W, L win^2)"""
    B, H, W, C = f1.shape
    L, r = c["L"], c["r"]
    fb = f2.shape[0]
    bmap = (torch.arange(B) * fb) // B if wrong == "f2_batch" else torch.arange(B) % fb
    bidx = bmap.view(B, 1).expand(B, H * W).reshape(-1)
    f1n = f1.reshape(B * H * W, C)
    isc = (1.0 / C) if wrong == "inv_c" else float(torch.tensor(1.0 / math.sqrt(C), dtype=f1.dtype))      # (rounded once in fp32)
    pyr = [f2]
    for _ in range(L - 1):
        pyr.append(_pool(pyr[-1]))
    outs = []
    for l in range(L):
        f2l = pyr[l]
        if wrong == "level_reused" and L > 1 and l == L - 2:
            f2l = F.interpolate(pyr[L - 1].permute(0, 3, 1, 2), size=tuple(pyr[l].shape[1:3]), mode="nearest").permute(0, 2, 3, 1)
        cx, cy = _level_coords(flow, H, W, l, r, wrong)
        cx, cy = cx.reshape(-1), cy.reshape(-1)
        tab, _, _, _ = _table(f1n, f2l, bidx, cx, cy, r, mode, "clamp" if wrong == "border_clamp" else "zeros")
        o = _blend(tab * isc, cx, cy, r, (W >> l) == 1, (H >> l) == 1, wrong)
        outs.append(o.reshape(B, H, W, -1))
    return torch.cat(outs, -1)


def _corr_impl(op, c, inp, dtype=torch.float32, wrong=None, mode="f32"):
    t = {k: v.to(dtype) for k, v in inp.items()}
    if op == "corr":
        return _lookup(t["f1"], t["f2"], t["flow"], c, mode, wrong)
    f1, f2, flow = (t[k].clone().requires_grad_(True) for k in ("f1", "f2", "flow"))
    _lookup(f1, f2, flow, c, "f32", wrong).backward(t["dout"])
    return f1.grad, f2.grad, flow.grad[..., :2]


# ------------------------------------------------------------------------------------------------------------------ the models
def _model_coords(flow, c, l):
    """float64 level coordinates (cx, cy) and their fp32 uncertainty (dix, diy), 0 on an axis of size 1"""
    H, W, r = c["H"], c["W"], c["r"]
    cx, cy = _level_coords(flow, H, W, l, r)
    Hl, Wl = H >> l, W >> l
    dix = 4 * U * torch.maximum(cx.abs(), torch.full_like(cx, Wl - 1.0)) * (Wl > 1)
    diy = 4 * U * torch.maximum(cy.abs(), torch.full_like(cy, Hl - 1.0)) * (Hl > 1)
    return cx.reshape(-1), cy.reshape(-1), dix.reshape(-1), diy.reshape(-1)


def _abs_pyramid(f2, L):
    pyr = [f2.abs()]
    for _ in range(L - 1):
        pyr.append(_pool(pyr[-1]))
    return pyr


def _corr_model(op, c, inp, mode="f32"):
    d = {k: v.double() for k, v in inp.items()}
    B, H, W, C = d["f1"].shape
    L, r = c["L"], c["r"]
    win, tw = 2 * r + 1, 2 * r + 2
    fb = d["f2"].shape[0]
    bsel = torch.arange(B) % fb
    isc = 1.0 / math.sqrt(C)
    if op == "corr":
        ref, vols = ref_forward(d["f1"], d["f2"][bsel], d["flow"], L, r)
        f1a = d["f1"].abs().reshape(B, H * W, C)
        A = torch.einsum("bpc,bqc->bpq", f1a, d["f2"].abs()[bsel].reshape(B, H * W, C)).reshape(B * H * W, 1, H, W) * isc
        s1 = f1a.sum(-1).reshape(-1, 1, 1, 1)
        s2 = d["f2"].abs().sum(-1)[bsel].unsqueeze(1)                                     # (B, 1, H, W)
        dlt = torch.arange(-r, r + 1, dtype=torch.float64)
        ms = []
        for l in range(L):
            if l:
                A, s2 = F.avg_pool2d(A, 2), F.avg_pool2d(s2, 2)
            Hl, Wl = A.shape[-2:]
            tb = (eb.TAU[mode] + (3 * l + 1) * U) * A
            if mode != "f32":
                tb = tb + eb.FLOOR_ACT * isc * (s1 + s2.repeat_interleave(H * W, 0))
            cx, cy, dix, diy = _model_coords(d["flow"], c, l)
            n = cx.numel()
            # the sample points: the reference's, offset AFTER the de-normalised centre (equal in exact arithmetic; 0 on an axis of size 1)
            ix = ((cx.view(n, 1, 1) + dlt.view(1, win, 1)) * (Wl > 1)).expand(n, win, win)
            iy = ((cy.view(n, 1, 1) + dlt.view(1, 1, win)) * (Hl > 1)).expand(n, win, win)
            ex, ey = dix.view(n, 1, 1).expand_as(ix), diy.view(n, 1, 1).expand_as(iy)
            S, cond = kb._slopes(vols[l].detach().permute(0, 2, 3, 1), iy, ix, ey, ex, "zeros")
            tbs = kb._bilinear(tb.permute(0, 2, 3, 1), iy, ix, "zeros")[0]
            # second order: where both coordinates sit on an integer whose other tap row AND column are outside (a border flow at a corner)
            # both slopes vanish and the fp32 value is eps_x eps_y t: dix diy x the largest tap sum of the cells the box touches
            img = vols[l].detach().permute(0, 2, 3, 1).abs()
            second = torch.zeros_like(S)
            for sx_ in (-1, 1):
                for sy_ in (-1, 1):
                    taps = kb._bilinear(img, iy + sy_ * ey, ix + sx_ * ex, "zeros")[1]
                    second = torch.maximum(second, taps[0] + taps[1] + taps[2] + taps[3])
            second = second * (ex * ey).unsqueeze(-1)
            ms.append((tbs + 7 * U * S + cond + second).reshape(B, H, W, win * win))
        m = torch.cat(ms, -1)
        return ref, torch.where(_bad(d["flow"]).unsqueeze(-1), torch.zeros((), dtype=m.dtype), m)
    # ---- the adjoint
    assert fb == B
    f1, f2, flow = (d[k].clone().requires_grad_(True) for k in ("f1", "f2", "flow"))
    out, _ = ref_forward(f1, f2, flow, L, r)
    out.backward(d["dout"])
    ref = (f1.grad, f2.grad, flow.grad[..., :2])
    ado = d["dout"].abs().reshape(B * H * W, L, win, win)
    f1n, f1a = d["f1"].reshape(-1, C), d["f1"].abs().reshape(-1, C)
    bidx = torch.arange(B).view(B, 1).expand(B, H * W).reshape(-1)
    pyr, apyr = [d["f2"]], _abs_pyramid(d["f2"], L)
    for _ in range(L - 1):
        pyr.append(_pool(pyr[-1]))
    k1 = cs(tw * tw * L) + 8
    m_f1 = torch.zeros(B * H * W, C, dtype=torch.float64)
    lev_abs, lev_cnt, lev_sens = [], [], []
    m_fl = torch.zeros(B * H * W, 2, dtype=torch.float64)
    near = torch.zeros(B * H * W, 2, dtype=torch.bool)
    bad = _bad(d["flow"]).reshape(-1)

    def level(l, idx, cx, cy, dix, diy):
        """the models of level l for the pixels idx with the level coordinates (cx, cy): (df1 rows, scattered |contribution|, scattered
        sensitivity, scattered count, dflow x, dflow y)"""
        Hl, Wl = H >> l, W >> l
        flat_x, flat_y = Wl == 1, Hl == 1
        n = cx.numel()
        e = lambda v: v.view(n, 1, 1)   # noqa: E731
        wx1, wy1 = e(cx - torch.floor(cx)), e(cy - torch.floor(cy))
        wx0, wy0 = 1 - wx1, 1 - wy1
        g, bi = ado[idx, l], bidx[idx]
        # W[n, dy, dx]: the adjoint weights of the table positions (|dout| through the blend), and their coordinate sensitivities
        z = torch.zeros(n, tw, tw, dtype=torch.float64, requires_grad=True)
        t00, t01, t10, t11 = _corners(z, r, flat_x, flat_y)
        val = t00 * (wx0 * wy0) + t01 * (wx1 * wy0) + t10 * (wx0 * wy1) + t11 * (wx1 * wy1)
        sens = (e(dix) * (wy0 * (t00 + t01) + wy1 * (t10 + t11)) + e(diy) * (wx0 * (t00 + t10) + wx1 * (t01 + t11))
                + e(dix * diy) * (t00 + t01 + t10 + t11))
        Wv, = torch.autograd.grad(val, z, g, retain_graph=True)
        Ws, = torch.autograd.grad(sens, z, g)
        _, inside, qyc, qxc = _table(f1n[idx, :1], pyr[l][..., :1], bi, cx, cy, r, "f32")
        Wv, Ws = Wv * inside * isc, Ws * inside * isc
        Ga = apyr[l][bi.view(-1, 1, 1), qyc[:, :, None], qxc[:, None, :]]                # pool_l(|f2|) at the table positions (n, tw, tw, C)
        rows = U * (k1 + 3 * l) * torch.einsum("nyx,nyxc->nc", Wv, Ga) + torch.einsum("nyx,nyxc->nc", Ws, Ga)
        # df2_l: scatter of |W| |f1| to the positions, the count of (pixel, position) pairs
        lin = ((bi.view(-1, 1, 1) * Hl + qyc[:, :, None]) * Wl + qxc[:, None, :]).reshape(-1)
        sc_ = lambda Wt: torch.zeros(B * Hl * Wl, C, dtype=torch.float64).index_add_(   # noqa: E731
            0, lin, (Wt.reshape(n, tw * tw, 1) * f1a[idx].view(n, 1, C)).reshape(-1, C)).view(B, Hl, Wl, C)
        cnt = torch.zeros(B * Hl * Wl, dtype=torch.float64).index_add_(0, lin, (inside & (Wv > 0)).reshape(-1).double()).view(B, Hl, Wl, 1)
        # dflow
        T = _table(f1n[idx], pyr[l], bi, cx, cy, r, "f32")[0] * isc
        Ab = _table(f1a[idx], apyr[l], bi, cx, cy, r, "f32")[0] * isc
        a, b, cc, dd = _corners(Ab, r, flat_x, flat_y)
        ta, tb_, tc, td = _corners(T, r, flat_x, flat_y)
        kf = U * (cs(C) + 8 + 3 * l)
        mixed = (g * ((tb_ - ta) - (td - tc)).abs()).sum((1, 2))
        mx = kf * (g * (wy0 * (a + b) + wy1 * (cc + dd))).sum((1, 2)) + diy * mixed
        my = kf * (g * (wx0 * (a + cc) + wx1 * (b + dd))).sum((1, 2)) + dix * mixed
        return rows, sc_(Wv), sc_(Ws), cnt, (0.0 if flat_x else 1.0) * mx / 2 ** l, (0.0 if flat_y else 1.0) * my / 2 ** l

    for l in range(L):
        Hl, Wl = H >> l, W >> l
        cx, cy, dix, diy = _model_coords(d["flow"], c, l)
        every = torch.arange(cx.numel())
        rows, sa, ss, cnt, mx, my = level(l, every, cx, cy, dix, diy)
        nr = lambda v, size: ((v - torch.round(v)).abs() < 1e-4) & (v > -(r + 1.5)) & (v < size + r + 0.5) & (size > 1)   # noqa: E731
        nx, ny = nr(cx, Wl) & ~bad, nr(cy, Hl) & ~bad
        near[:, 0] |= nx
        near[:, 1] |= ny
        idx = torch.nonzero(nx | ny).reshape(-1)
        if idx.numel():
            # a coordinate this close to an integer may fall into either cell in fp32: the models of the four cells around it, the largest
            # per pixel (df1, dflow) and all of them added to the elements they reach (df2)
            for sx_ in (-2e-4, 2e-4):
                for sy_ in (-2e-4, 2e-4):
                    r2, a2, s2, c2, x2, y2 = level(l, idx, cx[idx] + sx_ * (Wl > 1), cy[idx] + sy_ * (Hl > 1), dix[idx], diy[idx])
                    rows[idx], mx[idx], my[idx] = torch.maximum(rows[idx], r2), torch.maximum(mx[idx], x2), torch.maximum(my[idx], y2)
                    sa, ss, cnt = sa + a2, ss + s2, cnt + c2
        m_f1 += rows
        m_fl[:, 0] += mx
        m_fl[:, 1] += my
        lev_abs.append(sa)
        lev_sens.append(ss)
        lev_cnt.append(cnt)
    jump = torch.zeros(B * H * W, 2, dtype=torch.float64)
    if bool(near.any()):
        # the one-sided derivatives: the float64 reference with the flow moved to either side along that axis alone, level by level (in fp32
        # every level falls to its own side, so the jumps of the levels add up in absolute value)
        # ... and the reference itself round-trips every window offset on its own, so the offsets of one level fall to different sides too:
        # the jumps are taken per (level, offset along that axis)
        nw = win * win
        for ax in (0, 1):
            groups = [slice(l * nw + k * win, l * nw + (k + 1) * win) if ax == 0 else slice(l * nw + k, (l + 1) * nw, win)
                      for l in range(L) for k in range(win)]
            sides = []
            for s_ in (-1e-3, 1e-3):
                fl = d["flow"].clone()
                fl[..., ax] += s_
                fl.requires_grad_(True)
                o = ref_forward(d["f1"], d["f2"], fl, L, r)[0]
                sides.append([torch.autograd.grad(o[..., g_], fl, d["dout"][..., g_], retain_graph=True)[0][..., ax].reshape(-1) for g_ in groups])
            jump[:, ax] = near[:, ax] * sum((a_ - b_).abs() for a_, b_ in zip(*sides))
    # df2: down the pooling chain's adjoint (0.25 per level to each of the four children)
    up = lambda t: 0.25 * F.interpolate(t.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)   # noqa: E731

    def chain(levs, weight=True):
        acc = levs[-1]
        for l in range(L - 2, -1, -1):
            u_ = up(acc) * (1.0 if weight else 4.0)
            full = torch.zeros_like(levs[l])
            full[:, :u_.shape[1], :u_.shape[2]] = u_
            acc = levs[l] + full
        return acc

    A2, S2, M2 = chain(lev_abs), chain(lev_sens), chain(lev_cnt, weight=False) + L
    m_f2 = U * (M2 + 12) * A2 + S2
    m_f2_det = U * (M2.clamp_max(16) + 8 + L) * A2 + S2 + M2 * 2.0 ** -41 + U * ref[1].abs()
    zero = torch.zeros((), dtype=torch.float64)
    m_f1 = torch.where(bad.view(-1, 1), zero, m_f1).view(B, H, W, C)
    m_fl = torch.where(bad.view(-1, 1), zero, m_fl).view(B, H, W, 2)
    return ref, (m_f1, m_f2, m_fl), (m_f1, m_f2_det, m_fl), near.view(B, H, W, 2), jump.view(B, H, W, 2)


def _corr_reference(op, c, inp, mode="f32", det=False):
    """(ref, bound) = (torch's float64 result, margin x model); model() also returns the un-margined pieces"""
    if op == "corr":
        ref, m = _corr_model(op, c, inp, mode)
        return ref, MARGIN["corr:" + mode] * m
    ref, m, md, _, jump = _corr_model(op, c, inp)
    k = MARGIN["corr_bwd_det"] if det else MARGIN["corr_bwd"]
    m = md if det else m
    return ref, (k * m[0], k * m[1], k * m[2] + jump)            # (the one-sided jump is no rounding model: it takes no margin)


worst_ratio = kb.worst_ratio

# wrong variant -> the rule under which a case contains its error
_CORR_WRONG = {
    "corr": {
        "window_transposed": lambda c: True,
        "level_coord_half": lambda c: c["L"] > 1,
        "border_clamp": lambda c: c["kind"] in ("plus_border", "minus_border", "noisy"),
        "f2_batch": lambda c: 1 < c["fb"] < c["B"],
        "inv_c": lambda c: True,
        "level_reused": lambda c: c["L"] > 1,
        "flat_axis_as_today": lambda c: any(flat_axes(c)),
    },
    "corr_bwd": {
        "dflow_no_level_scale": lambda c: c["L"] > 1,
        "df2_missing_corner": lambda c: True,
        "flat_axis_gradient": lambda c: any(flat_axes(c)),
        "flat_axis_as_today": lambda c: any(flat_axes(c)),
    },
}


# ============================================================================================================== the loss kernels
# gather_normalize_kernel, xent_diag_kernel, flow_loss_kernel (csrc/pp_train.hip); pp_xent_diag_backward, pp_normalize_rows_backward with an
# index, pp_scatter_add_rows (csrc/pp_backward.hip); flow_loss_backward_kernel (csrc/pp_backward3.hip).  References from torch's float64
# F.normalize, F.cross_entropy, F.binary_cross_entropy_with_logits, F.interpolate(mode="nearest") and float64 autograd of those.  Models:
# * gather_normalize / normalize_bwd_indexed: kernel_bounds' normalize and normalize_bwd models with cs(C) (C up to 1024, rows through an index
#   with repeats, row_stride > C): u |q| (cs(C) + 4 + 1) (the kernel multiplies by a reciprocal: one rounding more than the division) and
#   u (cs(C) + 8) (|dq| + |q| sum |q dq|) / max(|x|, eps).  A zero row stays exactly zero.
# * xent_diag: row_loss[i] = mx + logf(sum_j expf(s L_ij - mx)) - s L_ii.  s L rounds once (u |s L|: for mx and for the diagonal), the final two
#   additions round once each (<= u (|mx| + |s L_ii| + |loss|) together with the former), expf and logf are 1 ulp (ocml), the argument's
#   rounding u |s L_ij - mx| is weighted by p_ij (<= the spread, bounded here by the 6), the sum of n positive terms cs(n) u relative in the
#   sum = cs(n) u ABSOLUTE after the log:   model = u (2 |mx| + 2 |s L_ii| + cs(n) + 6 + sum_j p_ij |s L_ij - mx| + |loss|)  — absolute: where the
#   diagonal dominates by 20 or 80 logit units the loss is 2e-9 resp. exactly 0 in fp32 and only this model, no relative bar, decides.
#   (The p-weighted spread is the correction to the issue's starting form: with logits of spread 30 at scale 10 the argument roundings of the
#   terms near the maximum alone exceed the constant 6.)  n = 1: exactly 0.
#   xent_diag_bwd: d_ij = (p_ij - [i == j]) up s / n: |up s / n| u (p_ij (6 + cs(n) + |s L_ij - mx| + |s L_ij| + sum_k p_ik |s L_ik|) + [i == j]) + u |d_ij| + TINY:
#   kernel_bounds' softmax model, whose inputs are exact, plus the rounding of s L_ij itself (u |s L_ij| in the exponent = relative in p_ij, and the
#   same of every term of the sum, weighted by its share: the correction to the issue's starting form, which the scale-10 cases need).
# * flow_loss: the three sums (BCE-with-logits, valid-weighted L1, count), terms fp32, accumulation double: no n-dependent term.  BCE term
#   u (|z| + |z t| + 3 log1p(e^-|z|) + |term|); L1 u (3 |flow| + 4 |g|) per component (g = (H / 64) p - grid with H for BOTH axes; sizes are powers
#   of two, so H / 64 and its product are exact); the count is exact.  A pixel with 0 < | |g| - max_flow | <= 8 u max_flow may be decided either
#   way: its term and 1 are added to the L1 and count bounds (at most 0.1 % of a case; an exact tie |g| == max_flow is NOT exempt: strictly <).
#   flow_loss_bwd: dcert = kc (sigmoid(z) - t): 4 u |kc| + u |dcert|; dflow = +-kf or 0 exactly, except where 0 < |flow - g| <= 4 u (|flow| + |g|)
#   (the sign may differ: bound 2 |kf|) and at the threshold pixels above (bound |kf|); an exact tie flow == fl32(g) gives exactly 0.
# * scatter_add_rows: no arithmetic freedom: bit-equal to adding the rows in ascending i in fp32 (margin 0).
LOSS_OPS = ("gather_normalize", "normalize_bwd_indexed", "xent_diag", "xent_diag_bwd", "flow_loss", "flow_loss_bwd", "scatter_add_rows")
EPS_N = 1e-12
KP = 64

_set("gather_normalize", 0.228, 0.68)
_set("normalize_bwd_indexed", 0.163, 0.54)
_set("xent_diag", 0.527, 1.6)
_set("xent_diag_bwd", 0.793, 2.4)
_set("flow_loss", 0.152, 0.46)
_set("flow_loss_bwd", 0.41, 1.25)
MEASURED["scatter_add_rows"], MARGIN["scatter_add_rows"] = 0.0, 0.0

_NC = [(n, C) for n in (1, 3, 4, 5, 257) for C in (1, 63, 64, 65, 96, 384, 1000, 1024)]
_LOSS_CASES = {
    "gather_normalize": [dict(n=n, C=C) for n, C in _NC],
    "normalize_bwd_indexed": [dict(n=n, C=C) for n, C in _NC if C in (1, 65, 96, 384, 1024)],
    "xent_diag": [dict(n=n, ld=n + pad, scale=s) for n in (1, 2, 63, 64, 65, 257, 1025) for pad in (0, 3) for s in (1.0, 10.0)],
    "xent_diag_bwd": [dict(n=n, ld=n + pad, scale=s) for n in (1, 2, 63, 64, 65, 257, 1025) for (pad, s) in ((0, 10.0), (3, 1.0))],
    "flow_loss": [dict(B=B, H=H, W=W, max_flow=mf, fill=fill) for (B, H, W) in ((2, 16, 16), (1, 32, 32), (2, 64, 64), (1, 16, 32), (1, 128, 128), (3, 1, 1))
                  for mf in (400.0, 5.3) for fill in ("mixed",)]
    + [dict(B=1, H=16, W=16, max_flow=5.3, fill="none"), dict(B=1, H=16, W=16, max_flow=5.3, fill="all")]
    # (three pixels are three roundings, not a random walk of thousands: the smallest shape sets the margin of the sums, so it is drawn 8 x)
    + [dict(B=3, H=1, W=1, max_flow=5.3, fill="mixed", draw=k) for k in range(1, 8)],
    "scatter_add_rows": [dict(n=n, C=C) for n in (1, 3, 4, 5, 257) for C in (1, 63, 64, 65, 384)],
}
_LOSS_CASES["flow_loss_bwd"] = _LOSS_CASES["flow_loss"]


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _loss_inputs(op, c, seed=0):
    g = kb._gen(9000 + 100 * LOSS_OPS.index(op) + seed + sum(int(v * 7) if isinstance(v, (int, float)) else len(v) for v in c.values()))
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    if op in ("gather_normalize", "normalize_bwd_indexed", "scatter_add_rows"):
        n, C = c["n"], c["C"]
        R = max(n // 2, 4)                                               # fewer rows than indices: repeats
        index = torch.randint(0, R, (n,), generator=g)
        index[:3] = torch.arange(3)[:n]
        if op == "scatter_add_rows":
            return dict(src=kb._upstream(g, (n, C)), index=index, rows=torch.tensor(R))
        stride = C + 3
        src = rn(R, stride) * (10.0 ** (torch.rand(R, 1, generator=g) * 4 - 2))
        if op == "gather_normalize":
            src[0, :C] = 0.0                                             # a zero row stays zero
        src[1, :C] *= 1e-20 / float(src[1, :C].double().norm())         # norm 1e-20: divided by eps
        src[2, :C] *= 1e-10 / float(src[2, :C].double().norm())         # norm 1e-10: where eps ADDED to the norm would show
        d = dict(src=src, index=index)
        if op == "normalize_bwd_indexed":
            d["dq"] = kb._upstream(g, (n, C))
        return d
    if op in ("xent_diag", "xent_diag_bwd"):
        n, ld, s = c["n"], c["ld"], c["scale"]
        Lg = rn(n, ld) * (3.0 / s)                                       # logits s L of spread 3 ...
        if n > 8:
            Lg[n // 2] *= 10.0                                           # ... one row of spread 30
            for i, dom in ((0, 5.0), (1, 20.0), (2, 80.0)):              # rows whose diagonal dominates by 5, 20, 80 logit units
                row = Lg[i, :n].clone()
                row[i] = float("-inf")
                Lg[i, i] = float(row.max()) + dom / s
        d = dict(L=Lg)
        if op == "xent_diag_bwd":
            d["up"] = torch.tensor([0.37])
        return d
    if op in ("flow_loss", "flow_loss_bwd"):
        B, H, W = c["B"], c["H"], c["W"]
        mf = f32(c["max_flow"])
        k = H / KP
        ys, xs = torch.meshgrid(torch.arange(KP, dtype=torch.float32), torch.arange(KP, dtype=torch.float32), indexing="ij")
        # key-point n = ix * 64 + iy holds the target of source cell (iy, ix): near its own cell (|g| of a few pixels: both sides of 5.3)
        base = torch.stack([xs.t(), ys.t()], -1).reshape(1, KP * KP, 2) * 1.0          # [ix * 64 + iy] = (ix, iy) in cell units
        pts = base + rn(B, KP * KP, 2) * (3.0 / k) + 0.25
        keep = torch.rand(B, KP * KP, generator=g)
        frac = {"mixed": 0.4, "none": 1.1, "all": -1.0}[c["fill"]]
        pts[keep < frac] = -1.0
        if c["fill"] == "mixed" and B > 1:
            pts[0] = -1.0 if H == 16 else pts[0]                        # (one image with every key-point invalid)
        pts[keep.roll(1, 1) < 0.05 * (c["fill"] == "mixed"), 1] = -1.0  # (only ONE coordinate -1: invalid as well)
        flow, cert = rn(B, H, W, 2) * 3, rn(B, H, W) * 4
        if c["fill"] != "none" and H >= 16:
            # planted at pixel (b = B - 1, y = 0, x = 0), key-point 0: |g| == max_flow exactly (g = (max_flow, 0): not counted, strictly <)
            pts[B - 1, 0] = torch.tensor([mf / k, 0.0])
            # planted at pixel (y = 0, x = W - 1): an exact tie flow == fl32(g)
            n_ = ((W - 1) * KP // W) * KP
            pts[B - 1, n_] = torch.tensor([(W - 1 + 1.5) / k, 2.25 / k])
            flow[B - 1, 0, W - 1] = torch.tensor([1.5, 2.25])
        d = dict(flow=flow, cert=cert, pts=pts)
        if op == "flow_loss_bwd":
            d["gf"], d["gc"] = torch.tensor([0.013]), torch.tensor([0.0007])
        return d
    raise ValueError(op)


def _flow_maps(c, pts, dt, wrong=None):
    """(gx, gy, valid) as (B, H, W) maps in dtype dt: the key-point grid brought to the map by nearest-neighbour interpolation"""
    B, H, W = c["B"], c["H"], c["W"]
    grid = pts.to(dt).view(B, KP, KP, 2)                                 # [ix, iy]
    grid = grid.permute(0, 3, 1, 2) if wrong == "keypoint_transposed" else grid.permute(0, 3, 2, 1)      # -> (B, 2, iy, ix)
    m = F.interpolate(grid, size=(H, W), mode="nearest")
    valid = (m[:, 0] != -1) & (m[:, 1] != -1)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    zero = torch.zeros((), dtype=dt)
    kx = (W / KP) if wrong == "w_for_x" else (H / KP)
    gx = torch.where(valid, kx * m[:, 0], zero) - xs
    gy = torch.where(valid, (H / KP) * m[:, 1], zero) - ys
    return gx, gy, valid


def _seq_scatter(src, index, rows):
    out = torch.zeros(rows, src.shape[1], dtype=src.dtype)
    for i in range(src.shape[0]):                                        # ascending i, one rounding per addition
        out[index[i]] += src[i]
    return out


def _loss_impl(op, c, inp, dtype=torch.float32, wrong=None, mode="f32"):
    t = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in inp.items()}
    if op in ("gather_normalize", "normalize_bwd_indexed"):
        idx = torch.arange(c["n"]) % t["src"].shape[0] if wrong == "index_ignored" else t["index"]
        x = t["src"][idx, :c["C"]]
        nrm = torch.sqrt((x * x).sum(1, keepdim=True))
        nrm = nrm + EPS_N if wrong == "eps_added" else nrm.clamp_min(EPS_N)
        if op == "gather_normalize":
            return x * (1.0 / nrm)
        q = x / nrm
        return t["dq"] / nrm if wrong == "no_projection" else (t["dq"] - q * (q * t["dq"]).sum(1, keepdim=True)) / nrm
    if op in ("xent_diag", "xent_diag_bwd"):
        n, s = c["n"], c["scale"]
        z = t["L"][:, :n] * s
        i = torch.arange(n)
        mx = z.max(1, keepdim=True).values
        if wrong == "no_max":
            mx = torch.zeros_like(mx)
        nn = (n // 64) * 64 if wrong == "tail_dropped" else n
        e = torch.exp(z - mx)
        ssum = e[:, :nn].sum(1, keepdim=True)
        if op == "xent_diag":
            return (mx + torch.log(ssum))[:, 0] - z[i, (i + 1) % n if wrong == "label_next" else i]
        k = t["up"][0] * s / (1.0 if wrong == "no_1_over_n" else float(n))
        delta = torch.zeros_like(z) if wrong == "no_delta" else torch.eye(n, dtype=dtype)
        return (e / ssum - delta) * k
    if op in ("flow_loss", "flow_loss_bwd"):
        gx, gy, valid = _flow_maps(c, t["pts"], dtype, wrong)
        mf = f32(c["max_flow"])
        z, tt = t["cert"], (torch.ones_like(t["cert"]) if wrong == "mask_ignored" else valid.to(dtype))
        mag = torch.sqrt(gx * gx + gy * gy)
        use = valid & ((mag <= mf) if wrong == "le_threshold" else (mag < mf))
        e0, e1 = t["flow"][..., 0] - gx, t["flow"][..., 1] - gy
        if op == "flow_loss":
            bce = z.clamp_min(0) - z * tt + torch.log1p(torch.exp(-z.abs()))
            l1 = torch.where(use, e0.abs() + e1.abs(), torch.zeros((), dtype=dtype))
            return torch.stack([bce.double().sum(), l1.double().sum(), use.double().sum()])
        kf, kc = t["gf"][0], t["gc"][0]
        dcert = kc * (1.0 / (1.0 + torch.exp(-z)) - tt)
        dflow = torch.stack([torch.sign(e0), torch.sign(e1)], -1) * kf * use.unsqueeze(-1)
        return dflow, dcert
    if op == "scatter_add_rows":
        src = t["src"]
        if wrong == "descending":
            return _seq_scatter(src.flip(0), t["index"].flip(0), int(t["rows"]))
        return _seq_scatter(src, t["index"], int(t["rows"]))
    raise ValueError(op)


def _loss_model(op, c, inp, mode="f32"):
    """(ref, model) of a loss kernel; flow_loss / flow_loss_bwd also return the exempt masks"""
    d = {k: (v.double() if v.is_floating_point() else v) for k, v in inp.items()}
    if op == "gather_normalize":
        q = F.normalize(d["src"][d["index"], :c["C"]], dim=1, eps=EPS_N)
        return q, U * q.abs() * (cs(c["C"]) + 5)
    if op == "normalize_bwd_indexed":
        x = d["src"][d["index"], :c["C"]].clone().requires_grad_(True)
        q = F.normalize(x, dim=1, eps=EPS_N)
        q.backward(d["dq"])
        q, dq = q.detach(), d["dq"]
        nrm = x.detach().norm(dim=1, keepdim=True).clamp_min(EPS_N)
        return x.grad, U * (cs(c["C"]) + 8) * (dq.abs() + q.abs() * (q * dq).abs().sum(1, keepdim=True)) / nrm
    if op in ("xent_diag", "xent_diag_bwd"):
        n, s = c["n"], c["scale"]
        Lg = d["L"][:, :n].clone().requires_grad_(True)
        z = Lg * s
        tgt = torch.arange(n)
        loss = F.cross_entropy(z, tgt, reduction="none")
        zd = z.detach()
        mx = zd.max(1, keepdim=True).values
        p = torch.softmax(zd, 1)
        dist = mx - zd
        if op == "xent_diag":
            m = U * (2 * mx[:, 0].abs() + 2 * zd[tgt, tgt].abs() + cs(n) + 6 + (p * dist).sum(1) + loss.detach().abs())
            return loss.detach(), m
        (loss.mean() * d["up"][0]).backward()
        k = float(d["up"][0]) * s / n
        zin = zd.abs() + (p * zd.abs()).sum(1, keepdim=True)              # s L_ij rounds before the subtraction: its own and the sum's terms'
        return Lg.grad, abs(k) * U * (p * (6 + cs(n) + dist + zin) + torch.eye(n, dtype=torch.float64)) + U * Lg.grad.abs() + kb.TINY
    if op in ("flow_loss", "flow_loss_bwd"):
        mf = f32(c["max_flow"])
        gx, gy, valid = _flow_maps(c, d["pts"], torch.float64)
        z, tt = d["cert"], valid.double()
        mag = torch.sqrt(gx * gx + gy * gy)
        use = valid & (mag < mf)
        edge = valid & ((mag - mf).abs() <= 8 * U * mf) & (mag != mf)          # either decision is accepted (an exact tie is not exempt)
        flow = d["flow"].clone().requires_grad_(True)
        zz = z.clone().requires_grad_(True)
        e0, e1 = flow[..., 0] - gx, flow[..., 1] - gy
        l1t = e0.abs() + e1.abs()
        bce = F.binary_cross_entropy_with_logits(zz, tt, reduction="sum")
        l1 = (l1t * use).sum()
        if op == "flow_loss":
            ref = torch.stack([bce.detach(), l1.detach(), use.double().sum()])
            bt = F.binary_cross_entropy_with_logits(z, tt, reduction="none")
            m_bce = (U * (z.abs() + (z * tt).abs() + 3 * torch.log1p(torch.exp(-z.abs())) + bt)).sum()
            m_l1 = (U * (3 * d["flow"].abs().sum(-1) + 4 * (gx.abs() + gy.abs())) * use).sum()
            extra = torch.stack([torch.zeros(()).double(), (l1t.detach() * edge).sum(), edge.double().sum()])
            return ref, torch.stack([m_bce, m_l1, torch.zeros(()).double()]), extra, edge
        kf, kc = float(d["gf"][0]), float(d["gc"][0])
        (kf * l1 + kc * bce).backward()
        sign_free = use.unsqueeze(-1) & (torch.stack([e0, e1], -1).detach().abs() <= 4 * U * (d["flow"].abs() + torch.stack([gx, gy], -1).abs())) \
            & (torch.stack([e0, e1], -1).detach() != 0)
        extra = 2 * abs(kf) * sign_free + abs(kf) * edge.unsqueeze(-1)
        m_c = 4 * U * abs(kc) + U * zz.grad.abs()
        return (flow.grad, zz.grad), (torch.zeros_like(flow.grad), m_c), (extra, torch.zeros_like(m_c)), (edge, sign_free)
    if op == "scatter_add_rows":
        want = _seq_scatter(inp["src"], inp["index"], int(inp["rows"])).double()
        return want, torch.zeros_like(want)
    raise ValueError(op)


def _loss_reference(op, c, inp, mode="f32", det=False):
    out = _loss_model(op, c, inp)
    ref, m = out[0], out[1]
    k = MARGIN[op]
    if op == "flow_loss":
        return ref, k * m + out[2]
    if op == "flow_loss_bwd":
        return ref, tuple(k * a + b for a, b in zip(m, out[2]))
    return ref, k * m


_LOSS_WRONG = {
    "gather_normalize": {"eps_added": lambda c: c["n"] >= 3, "index_ignored": lambda c: c["n"] >= 4},
    "normalize_bwd_indexed": {"no_projection": lambda c: c["C"] > 1, "index_ignored": lambda c: c["n"] >= 4},
    "xent_diag": {"label_next": lambda c: c["n"] > 1, "tail_dropped": lambda c: c["n"] % 64 != 0 and c["n"] > 64,
                  "no_max": lambda c: c["scale"] == 10.0 and c["n"] > 8},           # (evaluated in float32: expf overflows, below)
    "xent_diag_bwd": {"no_delta": lambda c: True, "no_1_over_n": lambda c: c["n"] > 1},
    "flow_loss": {"w_for_x": lambda c: c["H"] != c["W"], "keypoint_transposed": lambda c: c["H"] > 1 and c["fill"] == "mixed",
                  "mask_ignored": lambda c: c["fill"] != "all", "le_threshold": lambda c: c["fill"] != "none" and c["H"] >= 16 and c["max_flow"] == 5.3},
    "scatter_add_rows": {"descending": lambda c: c["n"] >= 257},                     # (evaluated in float32: the order is the only freedom)
}
# wrong variants whose effect exists in fp32 alone: xent_diag without the max subtraction is the same function in float64; in fp32 expf
# overflows once a logit exceeds 88.7, which only the scale-10 cases with the diagonal 80 logit units above the rest (row 2) reach
WRONG_IN_FP32 = {("xent_diag", "no_max"), ("scatter_add_rows", "descending")}


# ============================================================================================================== one table for both halves
CASES = {**_CORR_CASES, **_LOSS_CASES}
OPS = list(CASES)
WRONG = {**_CORR_WRONG, **_LOSS_WRONG}
_HALF = {op: (_corr_inputs, _corr_impl, _corr_model, _corr_reference) for op in _CORR_CASES}
_HALF.update({op: (_loss_inputs, _loss_impl, _loss_model, _loss_reference) for op in LOSS_OPS})


def inputs(op, c, seed=0):
    return _HALF[op][0](op, c, seed)


def impl(op, c, inp, dtype=torch.float32, wrong=None, mode="f32"):
    """the kernel's formula restated in torch in `dtype`; wrong: a structural error of WRONG[op]; mode: the lookup's arithmetic"""
    return _HALF[op][1](op, c, inp, dtype, wrong, mode)


def model(op, c, inp, mode="f32"):
    """(ref, un-margined model, ...): the lookup's adjoint adds (deterministic model, near-integer mask, one-sided jump), the flow loss its
    exemption allowance and masks"""
    return _HALF[op][2](op, c, inp, mode)


def reference(op, c, inp, mode="f32", det=False):
    """(ref, bound) = (torch's float64 result, MARGIN x model + the allowances that take no margin)"""
    return _HALF[op][3](op, c, inp, mode, det)
