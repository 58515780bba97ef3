"""Float64 references and componentwise error bounds for the contraction engine (pp_gemm: linear, convolution, transposed
convolution, batched products) in its three arithmetic modes.  A helper of the engine tests, imported through sys.path like
tests/netcfg.py; the references use torch's own float64 ops, never this project's kernels.

The check is elementwise:   |got - ref| <= bound,   with ref = the float64 result of the same op on the same fp32 inputs and

    bound = Lip * (tau * A + floor_a + floor_b + 2^-23 |b|) + eps_act + 2^-23 |act(.)|      (then LayerScale / residuals, below)
    A     = |x| (x) |w|           the same op on absolute values (|relu(x)| with relu_in), float64
    S_w   = 1 (x) |w|             per output element: sum over its k of |w_jk| (taps in the zero padding excluded)
    S_x   = |x| (x) 1             per output element: sum over its k of |x_ik|

Derivation of the constants (u16 = 2^-11: unit roundoff of fp16; u32 = 2^-24: of fp32):

* Activation operand (csrc/pp_common.h pp_split_f16, fixed scale PP_A_SCALE = 4, no per-tensor exponent): a = 4 x,
  hi = f16(a), lo = f16(a - hi).  a - hi is exact in fp32, |a - hi| <= u16 |a|, so |a - hi - lo| <= u16 |a - hi| <= 2^-22 |a|
  while lo is a normal fp16 number.  Once lo drops below 2^-14 (|a| below ~2^-3, |x| below ~2^-5) it is rounded on the fixed
  subnormal grid 2^-24: absolute error <= 2^-25 in a, i.e. 2^-27 in x.  So |x - (hi + lo) / 4| <= 2^-22 |x| + 2^-27: 22 bits
  for |x| >= 2^-5 and an absolute floor of 2^-27 per element below.  The "h" operand (f16 mode, pp_to_f16) is hi alone:
  <= u16 |x| + 2^-27.  The same holds for an operand the on-the-fly kernel (gemm_f16x3_kernel) splits from fp32, A or B.
* Weight operand (pp_split_weights_t / _ws): s = 2^e with e = clamp(10 - frexp_exponent(max|w|), -30, 30) (max|w| s in
  [512, 1024) unless the clamp binds; e = 0 for an all-zero weight), then the same hi / lo split of s w without the clamp at
  fp16's maximum.  Relative error as above (2^-22 hi + lo, u16 hi alone), absolute floor 2^-25 of s w = 2^-25 2^-e in w.
* f16x3 product (hi_a + lo_a)(hi_w + lo_w) - lo_a lo_w: each fp16 x fp16 product is exact in the fp32 MFMA accumulator, so the
  per-product error is the operand errors 2^-22 + 2^-22 plus the dropped lo_a lo_w <= 2^-22: about 2^-21 |x||w| with margin,
  plus |w| 2^-27 (floor_a) and |x| 2^-25 2^-e (floor_b).  fp32 accumulation in MFMA order adds about u32 sqrt(K)-ish of A on
  random data and at most a few u32 per K tile of a systematic drift; tau_f16x3 = 2^-18 = 8 x 2^-21 leaves the accumulation
  8x the emulated typical operand error (tests/test_engine_bounds_cpu.py measures 3-7e-8 of A for the split alone).
* f32 (v_mfma_f32_32x32x2_f32 or fp32 FMA): products rounded once (u32), fp32 accumulation: tau_f32 = 2^-18 as well (the fp32
  CPU result itself errs 2-4e-7 of A on these shapes), no floors.
* f16 (one fp16 MFMA per product): two 11-bit roundings, (1 + u16)^2 - 1 = 2^-10 + 2^-22 per product, plus the fp32 accumulation
  allowance of the other modes: tau_f16 = 2^-10 + 2^-18.  Floors as in f16x3.  A launch that does not take a pre-split A
  (N <= 64, unaligned rows, batched products) runs the on-the-fly f16x3 kernel, in f16 mode too (ops._fly_args): A is split there
  at activation scale, B is the hl weight operand with its scale when K % 8 == 0, else split as an activation as well: its floor
  is then the activation floor (b_fmt="act").
* A same-sign sum (x, w > 0) has no cancellation, so there the K-tile accounting is tested on its own: tau = 2^-16 (f32, f16x3).
  A K tile lost or counted twice moves the sum by a whole tile's share, 2^-9 of it at K = 16384 (32 k per tile in f16x3) and
  2^-8 in f16 (64 k per tile).  In f16 the per-product roundings (2^-11, unbiased) random-walk to ~2^-11 / sqrt(K) of the sum:
  the emulation measures 0.71 x 2^-16 at K = 16384, before fp32 accumulation, so f16 gets 2^-15 — still 2^-7 below a lost tile.
* Epilogue (csrc/pp_gemm_dev.h: out = residual + residual2 + gamma * act(alpha acc + bias), fp32): each add / multiply rounds
  once, <= u32 of its result; the bias, residual, residual2 and LayerScale terms are therefore charged 2^-23 (two roundings)
  of |b|, |res|, |res2|, |gamma act(pre)|, and the activation's own arithmetic 2^-23 of its output.  The pre-activation bound
  goes through the activation with its Lipschitz constant (1 for relu / leaky01 / tanh; GELU: max |d/dv v Phi(v)| = 1.129 ->
  1.13) and is scaled by |gamma|.  Approximation error of the activation itself: GELU = 0.5 v (1 + erf_rational(v / sqrt 2)),
  whose rational erf errs <= 4.2e-7 (pp_gemm_dev.h): 2e-6 absolute over |v| <= 10, the bar test_engine_gpu.py's
  test_gelu_epilogue_accuracy pins, plus 2^-23 |v| for the evaluation in fp32; tanh: device tanhf (ocml, a few ulp): 2^-22
  absolute (|tanh| < 1).
* Saturation: the operand formats hold |x| < 65504 / 4 = 16376 (and |s w| < 65504, which the weight scale guarantees); beyond,
  the producers clamp and OR bit 0 into the saturation word (ops.saturation_raised).

Every check prints the worst |err| / bound and where it occurred; WORST keeps the worst per mode for the run's summary.
"""
import math

import torch
import torch.nn.functional as F

if torch.get_num_threads() > 16:
    torch.set_num_threads(16)

TAU = {"f32": 2.0 ** -18, "f16x3": 2.0 ** -18, "f16": 2.0 ** -10 + 2.0 ** -18}
TAU_SAME_SIGN = {"f32": 2.0 ** -16, "f16x3": 2.0 ** -16, "f16": 2.0 ** -15}
FLOOR_ACT = 2.0 ** -27          # per activation element (|x| below 2^-5: the subnormal lo / h term at scale 4)
EPI = 2.0 ** -23                # two fp32 roundings of an epilogue term
LIP = {None: 1.0, "relu": 1.0, "leaky01": 1.0, "tanh": 1.0, "gelu": 1.13}
ACT_ERR = {None: 0.0, "relu": 0.0, "leaky01": 0.0, "tanh": 2.0 ** -22, "gelu": 2e-6}
ACT_F = {None: lambda t: t, "relu": F.relu, "gelu": F.gelu, "leaky01": lambda t: F.leaky_relu(t, 0.1), "tanh": torch.tanh}
WORST = {}                      # mode -> (worst ratio, case name)

# the dense (M, K, N) of the GPU sweep (tests/test_engine_bounds_gpu.py) and of its CPU emulation: every M in {1, 127, 128, 129, 255,
# 256, 257, 513}, N in {1, 2, 63, 64, 65, 127, 129, 255, 257} and K in {1, 8, 9, 31, 32, 33, 63, 64, 65, 392, 4097} occurs (K tile
# 32 in f16x3, 64 in f16; 392 % 16 == 8), plus the long-K (5, 16384, 1024)
DENSE = [
    (1, 1, 1), (127, 8, 2), (128, 9, 63), (129, 31, 64), (255, 32, 65), (256, 33, 127), (257, 63, 129), (513, 64, 255),
    (1, 65, 257), (127, 392, 257), (128, 4097, 129), (129, 392, 255), (255, 64, 129), (256, 32, 257), (257, 8, 255),
    (513, 392, 127), (513, 4097, 65), (127, 64, 64), (129, 1, 63), (255, 65, 2), (256, 392, 1), (1, 392, 65), (257, 32, 63),
    (128, 64, 129), (513, 8, 64), (1, 4097, 127), (255, 9, 257), (256, 31, 255), (127, 33, 129), (5, 16384, 1024),
]


def weight_exponent(w):
    """e of the weight operand scale 2^e (pp_split_weights_t): s max|w| in [512, 1024), clamped to [-30, 30]; 0 for all zeros."""
    m = float(w.abs().max()) if w.numel() else 0.0
    if not (m > 0.0 and math.isfinite(m)):
        return 0
    return max(-30, min(30, 10 - math.frexp(m)[1]))


def floor_w(w):
    """Absolute error per weight element of the pre-split weight operand: the subnormal lo term of s w, 2^-25 / s."""
    return 2.0 ** (-25 - weight_exponent(w))


def _apply(op, a, b, kw):
    if op == "linear":
        return F.linear(a, b)
    if op == "conv2d":
        return F.conv2d(a, b, stride=kw.get("stride", 1), padding=kw.get("padding", 0))
    if op == "conv_transpose2d":
        return F.conv_transpose2d(a, b, stride=kw["stride"])
    if op == "bmm_nt":
        return a @ b.transpose(-1, -2)
    if op == "bmm_nn":
        return a @ b
    raise ValueError(op)


def reference(op, x, w, mode, bias=None, act=None, gamma=None, residual=None, residual2=None, relu_in=False, alpha=1.0,
              b_fmt="weight", tau=None, device=None, **kw):
    """(ref, bound): float64 CPU tensors in the layout of the torch op (NCHW for convolutions).

    op: "linear" (x (M, K), w (N, K)) | "conv2d" (x NCHW, w (Cout, Cin, k, k), stride / padding) | "conv_transpose2d"
    (x NCHW, w (Cin, Cout, r, r), stride = r) | "bmm_nt" (x (.., M, K), w (.., N, K)) | "bmm_nn" (x (.., M, K), w (.., K, N)).
    b_fmt: "weight" (B pre-split with its power-of-two scale) | "act" (B split on the fly at activation scale).
    residual / residual2 in the output's layout.  device: where the float64 products run (default: the CPU, the GPU through
    torch's float64 path for large products)."""
    if device is None:    # large products: torch's float64 path on the GPU (never this project's kernels)
        big = x.numel() * (w.shape[0] if op == "linear" else w[0].numel()) > 2e8
        device = "cuda" if big and torch.cuda.is_available() else "cpu"
    dev = torch.device(device)
    xd = x.detach().to(dev, torch.float64)
    wd = w.detach().to(dev, torch.float64)
    if relu_in:
        xd = F.relu(xd)
    ref = _apply(op, xd, wd, kw) * alpha
    A = _apply(op, xd.abs(), wd.abs(), kw) * abs(alpha)
    bound = (TAU[mode] if tau is None else tau) * A
    del A
    if mode != "f32":
        s_w = _apply(op, torch.ones_like(xd), wd.abs(), kw)
        s_x = _apply(op, xd.abs(), torch.ones_like(wd), kw)
        fb = FLOOR_ACT if b_fmt == "act" else floor_w(w)
        bound = bound + abs(alpha) * (FLOOR_ACT * s_w + fb * s_x)
        del s_w, s_x
    ref, bound = ref.cpu(), bound.cpu()

    def chan(t):     # a per-output-channel vector broadcast over the output layout
        t = t.detach().cpu().double()
        return t.view(-1, 1, 1) if op in ("conv2d", "conv_transpose2d") else t

    if bias is not None:
        b = chan(bias)
        ref = ref + b
        bound = bound + EPI * b.abs()
    y = ACT_F[act](ref)
    bound = LIP[act] * bound + ACT_ERR[act] + EPI * y.abs() + (EPI * ref.abs() if act == "gelu" else 0.0)
    if gamma is not None:
        g = chan(gamma)
        y = g * y
        bound = g.abs() * bound + EPI * y.abs()
    for r in (residual, residual2):
        if r is not None:
            r = r.detach().cpu().double()
            y = y + r
            bound = bound + EPI * r.abs()
    return y, bound


def check(name, got, ref, bound, mode=None):
    """Assert |got - ref| <= bound elementwise; print the worst ratio and where it occurred.  Returns the worst ratio."""
    got = got.detach().cpu().double().contiguous()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    err = (got - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    i = int(ratio.argmax())
    worst = float(ratio.reshape(-1)[i])
    where = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    e, b = float(err.reshape(-1)[i]), float(bound.reshape(-1)[i])
    print(f"[bound] {mode or ''} {name}: worst |err|/bound = {worst:.3g} at {where} (err {e:.3g}, bound {b:.3g})", flush=True)
    if mode is not None and worst > WORST.get(mode, (-1.0, ""))[0]:
        WORST[mode] = (worst, name)
    assert worst <= 1.0, f"{name}: |err| / bound = {worst:.3g} at {where}: err {e:.3g} > bound {b:.3g} (ref {float(ref.reshape(-1)[i]):.6g})"
    return worst
