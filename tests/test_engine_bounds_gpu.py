"""Every path of the contraction engine (pp_gemm), each tile configuration pinned, against the float64 componentwise bound of
tests/engine_bounds.py (derivation there), in the three arithmetic modes.  The launch records of the engine (pp_prof_gemm_records2:
configuration, kind, A-delivery mode per launch) show which kernel produced each result: every case asserts that its launch used the
pinned configuration or the fall-back `gemm_plan` in csrc/pp_gemm.hip documents, and each family asserts the configurations it covered."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_bounds as eb  # noqa: E402

gpu = pytest.mark.gpu
ACTS = [None, "relu", "gelu", "leaky01", "tanh"]
PRESPLIT_CFGS = [0, 2, 4, 5, 6, 9, 10]      # 3 (alias of 4) and 7 / 8 (aliases of 0) are pinned on a few cases each
F32_CFGS = [0, 1, 2, 3, 4, 5, 6, 7]         # round-1 kernel 0 .. 2, fp32 engine 3 .. 7
ROUND1_CFGS = [0, 1, 2]


@pytest.fixture(scope="module", autouse=True)
def _worst_summary():
    yield
    for mode, (r, name) in sorted(eb.WORST.items()):
        print(f"[bound] worst |err|/bound in mode {mode}: {r:.3g} ({name})", flush=True)


@pytest.fixture(params=["f32", "f16x3", "f16"])
def mode(request, monkeypatch):
    from picopose_amd import ops

    monkeypatch.setattr(ops, "PRECISION", request.param)
    monkeypatch.setattr(ops, "WINOGRAD", False)          # the direct implicit-GEMM convolution (Winograd has its own tests)
    monkeypatch.setattr(ops, "WINOGRAD4", False)
    monkeypatch.delenv("PP_GEMM_FORCE_CFG", raising=False)
    ops.saturation_raised()
    yield request.param
    ops.drop_split_cache()


def _records():
    from picopose_amd import _lib

    cap = 64
    shape, ms = (ctypes.c_int * (8 * cap))(), (ctypes.c_float * cap)()
    fl, by, cnt = (ctypes.c_double * cap)(), (ctypes.c_double * cap)(), ctypes.c_int()
    _lib.check(_lib.lib().pp_prof_gemm_records2(cap, shape, ms, fl, by, ctypes.byref(cnt)), "pp_prof_gemm_records2")
    keys = ("M", "N", "K", "k", "cfg", "kind", "amode")
    return [dict(zip(keys, (shape[8 * i + j] for j in range(7)))) for i in range(cnt.value)]


def launched(fn, cfg):
    """fn() with PP_GEMM_FORCE_CFG = cfg (None: unpinned) -> (result, the engine's launch records of the call)."""
    from picopose_amd import _lib

    L = _lib.lib()
    old = os.environ.get("PP_GEMM_FORCE_CFG")
    if cfg is None:
        os.environ.pop("PP_GEMM_FORCE_CFG", None)
    else:
        os.environ["PP_GEMM_FORCE_CFG"] = str(cfg)
    _lib.check(L.pp_prof_gemm_enable(64), "pp_prof_gemm_enable")
    try:
        out = fn()
        torch.cuda.synchronize()
        recs = _records()
    finally:
        _lib.check(L.pp_prof_gemm_enable(0), "pp_prof_gemm_enable")
        if old is None:
            os.environ.pop("PP_GEMM_FORCE_CFG", None)
        else:
            os.environ["PP_GEMM_FORCE_CFG"] = old
    return out, recs


def u_expect(cfg, N, h_shape, vec):
    """The configuration a pinned pre-split launch records (csrc/pp_gemm.hip gemm_plan; a tail split 9 / 10 is recorded under its big tile
    5 / 4; the element-wise epilogue, vec false, exists for the 128-row tiles only)."""
    cfg = {9: 5, 10: 4, 3: 4, 7: 0, 8: 0, 1: 0}.get(cfg, cfg)
    if cfg == 6 and not (h_shape and N > 128):
        cfg = 5
    if cfg == 5 and N <= 128:
        cfg = 4
    if not vec and cfg != 2:
        cfg = 0
    return cfg


class Coverage:
    def __init__(self):
        self.seen = set()

    def note(self, rec, pinned, k=0, *, presplit, fvec, N, vec=True, h_shape=False, grouped=False):
        """Assert that the single record `rec` of a launch pinned to `pinned` is the expected kernel; remember what ran."""
        assert rec["k"] == k, ("not the direct implicit-GEMM launch", rec)
        if presplit:
            assert rec["kind"] == 0, rec
            assert rec["cfg"] == u_expect(pinned, N, h_shape, vec), (pinned, rec)
            self.seen |= {("u", rec["cfg"]), ("u_pinned", pinned), ("amode", rec["amode"])}
        else:
            assert rec["kind"] == 1, rec
            if fvec and (pinned >= 3 or grouped):
                want = 3 if pinned < 3 else pinned
                if rec["amode"] == 18 and want in (5, 7):   # natural-order convolutions: no 256x256 / 256x192 kernel, 256x128 runs
                    want = 4
                assert rec["cfg"] == want and rec["amode"] >= 16, (pinned, rec)
                self.seen.add(("f", rec["cfg"]))
            else:
                assert rec["cfg"] == pinned and 8 <= rec["amode"] <= 11, (pinned, rec)
                self.seen.add(("r1", rec["cfg"], bool(rec["amode"] & 2)))

    def require(self, *items):
        missing = [i for i in items if i not in self.seen]
        assert not missing, f"not covered: {missing} (seen {sorted(self.seen, key=str)})"


def _run_pinned(cov, name, fn, ref, bound, mode, cfgs, n_rec=1, **note):
    for cfg in cfgs:
        out, recs = launched(fn, cfg)
        assert len(recs) == n_rec, (name, cfg, recs)
        for r in recs:
            cov.note(r, cfg, **note)
        eb.check(f"{name} cfg {cfg}", out, ref, bound, mode)


def _path(mode, first_rec):
    """(presplit, arithmetic of the launch) from the record of a first, cfg-0 launch."""
    presplit = first_rec["kind"] == 0
    return presplit, (mode if presplit or mode == "f32" else "f16x3")   # the fp32-operand kernels split on the fly in f16 mode too


def _b_fmt(mode, presplit, K):
    return "weight" if presplit or K % 8 == 0 else "act"      # (ops._fly_args: hl weights with their scale in both modes)


def _dense_case(cov, mode, name, x, w, b=None, act=None, gamma=None, residual=None, tau=None, alias=None, xg=None):
    """x: the CPU input; xg: its device form when that is a strided view (default: x.cuda())."""
    from picopose_amd import ops

    M, K = x.shape
    N = w.shape[0]
    wg = w.cuda()
    xg = x.cuda() if xg is None else xg
    bg = None if b is None else b.cuda()
    gg, rg = (None if gamma is None else gamma.cuda()), (None if residual is None else residual.cuda())

    def fn():
        return ops.linear(xg, wg, bg, act=act, gamma=gg, residual=rg)

    _, first = launched(fn, 0)
    assert len(first) == 1, (name, first)
    presplit, arith = _path(mode, first[0])
    fvec = mode == "f32" and K % 4 == 0 and xg.stride(0) % 4 == 0 and act != "tanh"
    cfgs = (PRESPLIT_CFGS + ([alias] if alias else [])) if presplit else (F32_CFGS if fvec else ROUND1_CFGS)
    t = None if tau is None else tau[arith]
    ref, bound = eb.reference("linear", x, w, arith, bias=b, act=act, gamma=gamma, residual=residual, b_fmt=_b_fmt(mode, presplit, K),
                              tau=t)
    _run_pinned(cov, name, fn, ref, bound, mode, cfgs, presplit=presplit, fvec=fvec, N=N, vec=N % 8 == 0)
    return presplit


@gpu
def test_dense_sweep_every_configuration(mode):
    """Linear layers on the covering set of (M, K, N) edges (eb.DENSE), every activation, with and without bias, each under every
    tile configuration of its path; strided / column-slice rows with LayerScale and a residual; a same-sign long-K sum (lost or doubled K
    tiles); and the tail-split launches 9 / 10 on a shape where they do split."""
    cov = Coverage()
    for i, (M, K, N) in enumerate(eb.DENSE):
        g = torch.Generator().manual_seed(1000 + i)
        x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
        b = None if i % 3 == 2 else torch.randn(N, generator=g)
        act = ACTS[i % 5]
        _dense_case(cov, mode, f"linear {M}x{K}x{N} {act} bias={b is not None}", x, w, b, act, alias=(3, 7, 8)[i % 3])
    g = torch.Generator().manual_seed(1)
    wide = torch.randn(300, 3 * 64, generator=g)
    w, b = torch.randn(96, 64, generator=g) / 8, torch.randn(96, generator=g)
    gamma, res = torch.randn(96, generator=g), torch.randn(300, 96, generator=g)
    _dense_case(cov, mode, "column-slice rows + LayerScale + residual", wide[:, 64:128], w, b, "gelu", gamma=gamma, residual=res,
                xg=wide.cuda()[:, 64:128])                    # row stride 192
    wide2 = torch.randn(257, 392 + 24, generator=g)
    w2 = torch.randn(129, 392, generator=g) / 20
    _dense_case(cov, mode, "strided rows 257x392x129 no bias", wide2[:, 8:400], w2, None, "leaky01", xg=wide2.cuda()[:, 8:400])
    for M, K, N, act in ((257, 392, 136, "relu"), (513, 32, 264, None)):    # N % 8 == 0: the vector epilogue of the wide tiles
        x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
        _dense_case(cov, mode, f"linear {M}x{K}x{N} {act}", x, w, torch.randn(N, generator=g), act, alias=3)
    # same sign: every product adds, a K tile lost or counted twice is >= 2^-9 of the sum
    xp, wp = torch.rand(64, 16384, generator=g), torch.rand(256, 16384, generator=g) / 16384
    _dense_case(cov, mode, "same-sign K=16384", xp, wp, tau=eb.TAU_SAME_SIGN)
    # the tail split: whole rounds of 256-row tiles + the remaining rows on 128x128 tiles (a second launch, recorded with the first)
    M, K, N = 256 * 100 + 77, 256, 768
    xt, wt, bt = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / 16, torch.randn(N, generator=g)
    from picopose_amd import ops

    ref, bound = eb.reference("linear", xt, wt, mode, bias=bt, act="relu", device="cuda")
    xg, wg, bg = xt.cuda(), wt.cuda(), bt.cuda()
    if mode != "f32":
        _run_pinned(cov, "tail split", lambda: ops.linear(xg, wg, bg, act="relu"), ref, bound, mode, [9, 10], presplit=True, fvec=False, N=N)
    else:                # (the fp32 engine records the tail split under 5 / 4 as well)
        for cfg, want in ((9, 5), (10, 4)):
            out, recs = launched(lambda: ops.linear(xg, wg, bg, act="relu"), cfg)
            assert len(recs) == 1 and recs[0]["cfg"] == want and recs[0]["amode"] >= 16, recs
            eb.check(f"tail split cfg {cfg}", out, ref, bound, mode)
    if mode == "f32":
        cov.require(*[("f", c) for c in (3, 4, 5, 6, 7)], *[("r1", c, False) for c in ROUND1_CFGS])
    else:
        cov.require(*[("u", c) for c in (0, 2, 4, 5)], *[("u_pinned", c) for c in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10)], ("amode", 0),
                    *[("r1", c, True) for c in ROUND1_CFGS])


CONVS = [  # B, cin, cout, k, stride, pad, hw, extras
    (2, 3, 64, 7, 1, 3, 20, {}),                                   # Cin 3: scalar loads (fp32 operands)
    (2, 3, 64, 14, 14, 0, 28, {}),                                 # patch embed
    (2, 8, 96, 3, 2, 1, 17, {"act": "relu"}),                      # Cin 8, stride 2, partial tiles
    (3, 36, 130, 3, 1, 1, 13, {"relu_in": True, "res": 1}),        # Cin 36, column tail
    (2, 64, 256, 3, 1, 1, 16, {"res": 2, "act": "leaky01"}),       # Cin 64: channel-slice-major K; row-shared delivery (cfg 6)
    (3, 72, 136, 3, 1, 1, 20, {"act": "gelu"}),                    # Cin 72: natural K order
    (1, 640, 160, 3, 1, 1, 16, {}),                                # Cin 640, cfg 6
    (2, 64, 128, 1, 1, 0, 15, {"act": "tanh", "res": 1}),          # 1x1
    (5, 64, 96, 3, 1, 1, 8, {"relu_in": True}),                    # batch tails, small map
    (2, 64, 72, 7, 1, 3, 12, {"act": "relu"}),                     # 7x7 pad 3
]


def _conv_case(cov, mode, name, x, w, b, k, s, p, act=None, relu_in=False, res=0, split_in=False, slices=False):
    from picopose_amd import ops

    g = torch.Generator().manual_seed(x.shape[1] * 13 + w.shape[0])
    B, cin, H, W = x.shape
    cout = w.shape[0]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    r1 = torch.randn(B, cout, Ho, Wo, generator=g) if res >= 1 else None
    r2 = torch.randn(B, cout, Ho, Wo, generator=g) if res >= 2 else None
    wp, bg = ops.pack_conv_weight(w.cuda()), (None if b is None else b.cuda())
    rg1 = None if r1 is None else ops.to_nhwc(r1.cuda())
    rg2 = None if r2 is None else ops.to_nhwc(r2.cuda())
    if slices:     # channel slices: the input a slice of a wider NHWC map, the output written into a slice of another
        wide_in = torch.zeros(B, H, W, 3 * cin, device="cuda")
        wide_in[..., cin:2 * cin] = ops.to_nhwc(x.cuda())
        wide_out = torch.zeros(B, Ho, Wo, cout + 32, device="cuda")

        def fn():
            ops.conv2d(wide_in[..., cin:2 * cin], wp, bg, k, s, p, act=act, out=wide_out[..., 16:16 + cout], cin=cin)
            return wide_out[..., 16:16 + cout].permute(0, 3, 1, 2)
    else:
        xn = ops.to_nhwc(x.cuda())
        src = ops.split_image(xn) if split_in else xn
        assert not split_in or isinstance(src, ops.Split)

        def fn():
            return ops.to_nchw(ops.conv2d(src, wp, bg, k, s, p, act=act, relu_in=relu_in, residual=rg1, residual2=rg2))

    _, first = launched(fn, 0)
    assert len(first) == 1, (name, first)
    presplit, arith = _path(mode, first[0])
    K = k * k * cin
    ld = 3 * cin if slices else cin
    fvec = mode == "f32" and cin % 4 == 0 and ld % 4 == 0 and act != "tanh"
    kt = 64 // ops.terms() if presplit else 32
    h_shape = (k == 3 and s == 1 and p == 1 and cin % kt == 0 and H == W and 16 <= W <= 256 and W & (W - 1) == 0 and not slices)
    ldc = cout + 32 if slices else cout
    cfgs = [0, 2, 4, 5, 6] if presplit else (F32_CFGS if fvec else ROUND1_CFGS)
    ref, bound = eb.reference("conv2d", x, w, arith, bias=b, act=act, residual=r1, residual2=r2, relu_in=relu_in,
                              b_fmt=_b_fmt(mode, presplit, K), stride=s, padding=p)
    _run_pinned(cov, name, fn, ref, bound, mode, cfgs, k=k, presplit=presplit, fvec=fvec, N=cout, vec=cout % 8 == 0 and ldc % 4 == 0,
                h_shape=h_shape)
    if slices:
        assert not wide_out[..., :16].any() and not wide_out[..., 16 + cout:].any()


@gpu
def test_conv_direct_path_every_configuration_records_the_tile_that_ran(mode):
    """Direct (implicit-GEMM) convolutions, Winograd off: Cin 3 / 8 / 36 / 64 / 72 / 640, 1x1, 3x3 (stride 1 and 2), 7x7, the 14x14
    patch embed, partial tiles and batch tails, relu_in, residual and residual2, channel-slice input and output, an operand (Split)
    input; then the transposed convolution's pixel-shuffle store at r = 2 and 4.  Every record is a direct launch (conv kernel size k)
    and names the tile that ran: a natural-order convolution pinned to 5 / 7 on the fp32 engine runs, and is recorded as, 256x128 (4)."""
    from picopose_amd import ops

    cov = Coverage()
    for i, (B, cin, cout, k, s, p, hw, ex) in enumerate(CONVS):
        g = torch.Generator().manual_seed(2000 + i)
        x = torch.randn(B, cin, hw, hw, generator=g)
        w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
        b = None if i % 4 == 3 else torch.randn(cout, generator=g)
        _conv_case(cov, mode, f"conv {B}x{cin}->{cout} k{k}s{s}p{p} {hw}x{hw} {ex}", x, w, b, k, s, p, act=ex.get("act"),
                   relu_in=ex.get("relu_in", False), res=ex.get("res", 0))
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(2, 64, 16, 16, generator=g), torch.randn(64, 64, 3, 3, generator=g) / 24, torch.randn(64, generator=g)
    _conv_case(cov, mode, "conv channel-slice in / out", x, w, b, 3, 1, 1, slices=True)
    if mode != "f32":
        x, w = torch.randn(2, 64, 32, 32, generator=g), torch.randn(192, 64, 3, 3, generator=g) / 24
        _conv_case(cov, mode, "conv on a Split operand", x, w, b=None, k=3, s=1, p=1, act="relu", split_in=True)
    for r, cin, cout, hw in ((2, 64, 96, 12), (4, 32, 40, 8)):
        x = torch.randn(2, cin, hw, hw, generator=g)
        w, b = torch.randn(cin, cout, r, r, generator=g) / cin ** 0.5, torch.randn(cout, generator=g)
        wp, bp = ops.pack_convT_weight(w.cuda(), b.cuda())
        xn = ops.to_nhwc(x.cuda())

        def fn():
            return ops.to_nchw(ops.conv_transpose2d(xn, wp, bp, r))

        _, first = launched(fn, 0)
        presplit, arith = _path(mode, first[0])
        fvec = mode == "f32"
        ref, bound = eb.reference("conv_transpose2d", x, w, arith, bias=b, b_fmt=_b_fmt(mode, presplit, cin), stride=r)
        _run_pinned(cov, f"conv_transpose r={r} {cin}->{cout}", fn, ref, bound, mode, [0, 2, 4, 5] if presplit else F32_CFGS,
                    presplit=presplit, fvec=fvec, N=r * r * cout, vec=cout % 8 == 0)
    if mode == "f32":
        cov.require(*[("f", c) for c in (3, 4, 5, 6, 7)], *[("r1", c, False) for c in ROUND1_CFGS])
    else:
        cov.require(*[("u", c) for c in (0, 2, 4, 5, 6)], ("amode", 1), ("amode", 2), *[("r1", c, True) for c in ROUND1_CFGS])


@gpu
def test_batched_products(mode):
    """bmm_nt (with alpha) and bmm_nn on strided 4-D views with z = 6 (the on-the-fly kernels: both operands split at activation scale
    in the f16x3 / f16 modes), and the grouped fp32 batch (one launch of the fp32 engine whose row tiles read their own product's
    weights: PpGemmDesc.grp_rows)."""
    from picopose_amd import ops

    cov = Coverage()
    g = torch.Generator().manual_seed(5)
    B, T, h, hd = 2, 77, 3, 64
    qkv = torch.randn(B, T, 3, h, hd, generator=g)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    d = qkv.cuda()
    qd, kd, vd = (d[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    arith = "f32" if mode == "f32" else "f16x3"
    ref, bound = eb.reference("bmm_nt", q, k, arith, alpha=hd ** -0.5, b_fmt="act")
    _run_pinned(cov, "bmm_nt alpha", lambda: ops.bmm_nt(qd, kd, alpha=hd ** -0.5), ref, bound, mode, ROUND1_CFGS, presplit=False, fvec=False,
                N=T)
    s = torch.softmax(ref.float(), dim=-1)
    sd = s.cuda()
    o = torch.empty(B, T, h, hd, device="cuda")
    ref, bound = eb.reference("bmm_nn", s, v, arith, b_fmt="act")

    def nn():
        ops.bmm_nn(sd, vd, o.permute(0, 2, 1, 3))
        return o.permute(0, 2, 1, 3)

    _run_pinned(cov, "bmm_nn", nn, ref, bound, mode, ROUND1_CFGS, presplit=False, fvec=False, N=hd)
    cov.require(*[("r1", c, mode != "f32") for c in ROUND1_CFGS])
    if mode == "f32":     # the grouped batch: prec = 0 whatever the mode
        nb, M, N, K = 5, 512, 130, 36
        A = torch.randn(nb, M, K, generator=g)
        Wt = torch.randn(nb, N, K, generator=g) / K ** 0.5
        bias = torch.randn(N, generator=g)
        Ag, Wg, bg = A.cuda(), Wt.cuda(), bias.cuda()
        out = torch.full((nb, M, N), float("nan"), device="cuda")

        def fn():
            ops._run(ops._desc(A=ops._p(Ag), B=ops._p(Wg), C=ops._p(out), bias=ops._p(bg), M=M, N=N, K=K, lda=K, ldb=K, ldc=N, prec=0,
                               act=ops.ACT["relu"], batch0=nb, a_bs0=M * K, b_bs0=N * K, c_bs0=M * N))
            return out

        ref, bound = eb.reference("bmm_nt", A, Wt, "f32", bias=bias, act="relu")
        _run_pinned(cov, "grouped fp32 batch", fn, ref, bound, mode, [0, 3], presplit=False, fvec=True, N=N, grouped=True)
        cov.require(("f", 3))


def _mag_paths(mode):
    """(name, K, N) of the dense paths the magnitude edges run: pre-split (N > 64) and on-the-fly (N <= 64) in the f16x3 / f16 modes."""
    return [("presplit", 392, 257), ("on-the-fly", 392, 63)]


@gpu
def test_magnitude_edges(mode):
    """Activations scaled by 2^-20, 2^-8, 1, 2^8 and with max|x| = 16000 (just under the operand limit 16376): the bound with its floors
    holds and the saturation word stays clear.  Weights with max|w| = 2^-40 (the exponent clamp binds), 2^-20, 2^20, exactly 1 and the
    next float below (the frexp boundary), all zero (e = 0).  An all-zero input row gives exactly the bias.  On the pre-split and the
    on-the-fly path, and on a convolution from an fp32 map."""
    from picopose_amd import ops

    g = torch.Generator().manual_seed(11)
    cases = []
    for name, K, N in _mag_paths(mode):
        x0, w0 = torch.randn(257, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
        for sc in (2.0 ** -20, 2.0 ** -8, 1.0, 2.0 ** 8):
            cases.append((f"{name} x*2^{int(torch.tensor(sc).log2())}", x0 * sc, w0))
        xb = x0.clone()
        xb[3, 5] = 16000.0
        cases.append((f"{name} max|x|=16000", xb, w0))
        one_below = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
        for wmax in (2.0 ** -40, 2.0 ** -20, 2.0 ** 20, 1.0, one_below):
            ws = w0 / w0.abs().max() * wmax
            ws.view(-1)[7] = wmax                         # max|w| exactly wmax
            cases.append((f"{name} max|w|={wmax:.9g}", x0, ws))
        cases.append((f"{name} w=0", x0, torch.zeros(N, K)))
    for name, x, w in cases:
        b = torch.randn(w.shape[0], generator=g) if "w=" in name and "max" not in name else None
        xg, wg = x.cuda(), w.cuda()
        bg = None if b is None else b.cuda()
        out, recs = launched(lambda: ops.linear(xg, wg, bg), 0)
        assert len(recs) == 1
        presplit, arith = _path(mode, recs[0])
        ref, bound = eb.reference("linear", x, w, arith, bias=b, b_fmt=_b_fmt(mode, presplit, x.shape[1]))
        eb.check(f"magnitude {name}", out, ref, bound, mode)
        assert not ops.saturation_raised(), name
    # an all-zero input row: exactly the bias
    for name, K, N in _mag_paths(mode):
        x, w, b = torch.randn(129, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
        x[5] = 0.0
        out = ops.linear(x.cuda(), w.cuda(), b.cuda())
        assert torch.equal(out[5].cpu(), b), name
    # a convolution from an fp32 map at the magnitude edges of its activations
    x0, w = torch.randn(2, 64, 16, 16, generator=g), torch.randn(96, 64, 3, 3, generator=g) / 24
    wp = ops.pack_conv_weight(w.cuda())
    for sc in (2.0 ** -20, 2.0 ** -8, 2.0 ** 8):
        x = x0 * sc
        out = ops.to_nchw(ops.conv2d(ops.to_nhwc(x.cuda()), wp, None, 3, 1, 1))
        ref, bound = eb.reference("conv2d", x, w, mode, stride=1, padding=1)
        eb.check(f"magnitude conv x*{sc:g}", out, ref, bound, mode)
        assert not ops.saturation_raised()


@gpu
def test_saturation_word_on_every_operand_path(mode):
    """One activation element at 16400 (beyond |x| < 16376) sets the saturation word on the pre-split path, the on-the-fly split
    (including an operand B split on the fly: bmm_nt) and a convolution from an fp32 map; the strict-fp32 mode has no operand format and
    never sets it."""
    from picopose_amd import ops

    g = torch.Generator().manual_seed(12)
    x = torch.randn(129, 392, generator=g)
    x[3, 7] = 16400.0
    xg = x.cuda()
    wc = ops.pack_conv_weight((torch.randn(96, 64, 3, 3, generator=g) / 24).cuda())
    xc = torch.randn(2, 16, 16, 64, generator=g)
    xc[1, 4, 5, 6] = 16400.0
    qk = torch.randn(1, 2, 70, 64, generator=g)
    qk2 = qk.clone()
    qk2[0, 1, 9, 3] = 16400.0
    runs = [
        ("presplit linear", lambda: ops.linear(xg, (torch.randn(257, 392, generator=g) / 20).cuda())),
        ("on-the-fly linear", lambda: ops.linear(xg, (torch.randn(63, 392, generator=g) / 20).cuda())),
        ("conv from an fp32 map", lambda: ops.conv2d(xc.cuda(), wc, None, 3, 1, 1)),
        ("on-the-fly B operand", lambda: ops.bmm_nt(qk.cuda(), qk2.cuda())),
    ]
    for name, fn in runs:
        ops.saturation_raised()
        fn()
        assert ops.saturation_raised() == (mode != "f32"), (name, mode)
