"""The stage-2/3 geometry kernels (csrc/pp_geom.hip) and pp_simvol_backward through their Python wrappers — and straight through the C
ABI where the wrapper hides something (the adjoint's output buffer, the gather's padding rows and counts) — against the float64
references and derived bounds of tests/geom_bounds.py, over its sweep of shapes and edges.  Every case prints one [bound] line."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geom_bounds as gb  # noqa: E402

gpu = pytest.mark.gpu
kb, eb = gb.kb, gb.kb.eb
SENTINEL = 0x7FC5A5A5          # a quiet NaN with a payload: no kernel result has these bits


def _simvol_backward(out, dout, mask):
    """pp_simvol_backward into a buffer pre-filled with NaN: an element the kernel does not write stays NaN"""
    from picopose_amd import _lib

    B = out.shape[0]
    dS = torch.full((B, 256, 256), float("nan"), device="cuda")
    _lib.check(_lib.lib().pp_simvol_backward(out.data_ptr(), dout.data_ptr(), mask.data_ptr(), mask.shape[1], mask.shape[2], B, dS.data_ptr(),
                                             _lib.stream_ptr()), "pp_simvol_backward")
    return dS


def _gather_abi(feat, idx):
    """pp_gather_valid with `out` pre-filled with a sentinel bit pattern and `count` with -1 -> (counts, rows per item); asserts that
    the rows from `count` on still hold the sentinel"""
    from picopose_amd import _lib

    B, C, H, W = feat.shape
    N = idx.shape[1]
    out = torch.full((B, N, C), SENTINEL, dtype=torch.int32, device="cuda")
    count = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().pp_gather_valid(feat.data_ptr(), idx.data_ptr(), B, C, H, W, N, out.data_ptr(), count.data_ptr(), _lib.stream_ptr()),
               "pp_gather_valid")
    counts = count.cpu()
    assert bool(((counts >= 0) & (counts <= N)).all()), counts
    for b in range(B):
        assert bool((out[b, int(counts[b]):] == SENTINEL).all()), f"item {b}: rows beyond count = {int(counts[b])} were written"
    return counts, [out[b, :int(counts[b])].view(torch.float32).cpu() for b in range(B)]


def run_hip(op, inp):
    """the operation's outputs from the HIP kernels, in the structure geom_bounds.model returns"""
    from picopose_amd.utils.correspondence import compute_init_correspondences, compute_stage3_correspondences
    from picopose_amd.utils.matching import matching_features_similarity
    from picopose_amd.utils.pose_recovery import pose_recovery_2d_prediction
    from picopose_amd.utils.torch_utils import calc_pred_Ms

    t = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}
    if op == "simvol":
        return matching_features_similarity(t["src"], t["tar"], t["mask"], None)
    if op == "simvol_bwd":
        return _simvol_backward(t["out"], t["dout"], t["mask"])
    if op == "pred_ms":
        return calc_pred_Ms(t["scale"], t["inplane"], t["trans"], t["tem_pose"], t["tem_K"], t["tem_M"], trans_scale=t["trans_scale"])
    if op == "pose2d":
        return pose_recovery_2d_prediction(t["query_M"], t["query_K"], t["pred_Ms"], t["tem_K"], t["tem_M"], t["tem_pose"])
    if op == "init_corr":
        return compute_init_correspondences(t["pred_Ms"], t["mask"])
    if op == "stage3":
        return compute_stage3_correspondences(t["flow"], t["cert"], threshold=t["thr"])
    if op == "gather":
        return _gather_abi(t["feat"], t["idx"])
    raise ValueError(op)


@gpu
@pytest.mark.parametrize("op", gb.OPS)
def test_kernel_against_float64_bound(op):
    """Every case of the operation's sweep: |kernel - float64 reference| <= MARGIN x model element by element; bit-equal for the
    operations without arithmetic of their own (adjoint, stage-3 decisions outside the sigmoid band, gather)."""
    from picopose_amd.utils.torch_utils import gather

    for c in gb.CASES[op]:
        inp = gb.inputs(op, c)
        ref, bound = gb.reference(op, inp)
        got = run_hip(op, inp)
        name = gb.case_name(op, c)
        if op == "simvol":
            g, zero = got.cpu(), bound == 0                 # mask 0 or a column of zeros: exactly 0, not merely small
            assert bool((g[zero] == 0).all()), name
        if op == "simvol_bwd":
            assert not bool(torch.isnan(got).any()), f"{name}: {int(torch.isnan(got).sum())} elements of dS were never written"
        if op == "init_corr":
            assert torch.equal(got[1].cpu().double(), ref[1]), name
        if op == "stage3":
            for (b, h, w) in inp["planted"]:
                assert not bool(bound["exempt_bhw"][b, h, w])
        gb.check(op, name, got, ref, bound)
        if op == "gather":                                  # the wrapper: the valid rows of all items, concatenated in order
            assert torch.equal(gather(inp["feat"].cuda(), inp["idx"].cuda()).cpu(), torch.cat(ref[1], 0)), name
    w = gb.WORST.get(op)
    print(f"[worst] {op}: {w[0]:.3g} at {w[1]}" if w else f"[worst] {op}: -")


@gpu
def test_similarity_volume_adjoint_through_autograd_at_33_images():
    """autograd.similarity_volume at B = 33 (the first batch beyond the adjoint's grid cap of 8192 blocks = 32 images) against the
    float64 autograd of the float64 forward.  The bound is composed from the existing models: dS = dout m [out > 0] is one product
    (u |dS|), plus |dout m| where the forward value lies within its own bound of 0 (the mask may fall on either side); the two
    batched products dS xhat, dS^T qhat carry engine_bounds' bound on the range-normalised dS (on-the-fly f16x3 kernel, both
    operands split as activations) plus dS's and the normalised rows' (kernel_bounds "normalize") errors carried through; F.normalize's
    adjoint is kernel_bounds "normalize_bwd" on the product, with the product's error carried through the projection."""
    from picopose_amd import autograd as ag
    from picopose_amd import ops

    g = torch.Generator().manual_seed(33)
    B, P, C = 33, 256, 64
    ts, tt = torch.randn(B, P + 1, C, generator=g), torch.randn(B, P + 1, C, generator=g)
    mask = gb._mask(g, B, 37, 53)
    dout = torch.randn(B, 256, 16, 16, generator=g)

    # float64 autograd of the float64 forward
    a, b = ts.double().requires_grad_(True), tt.double().requires_grad_(True)
    xh, qh = F.normalize(a[:, 1:], dim=2), F.normalize(b[:, 1:], dim=2)          # (B, P, C)
    m = gb._nearest16_ref(mask).reshape(B, 1, P)
    pre = torch.einsum("btc,bsc->bts", qh, xh) * m
    gb._to_out_layout(F.relu(pre)).backward(dout.double())

    # the composed bound
    xh, qh, pre = xh.detach(), qh.detach(), pre.detach()
    nchw = lambda tok: tok[:, 1:].transpose(1, 2).reshape(B, C, 16, 16)   # noqa: E731
    fwd_bound = gb._from_out_layout(gb.reference("simvol", dict(src=nchw(ts), tar=nchw(tt), mask=mask))[1])
    d_ts = gb._from_out_layout(dout.double())                                       # dout as [b][t][s]
    G = torch.where(pre > 0, d_ts * m, torch.zeros((), dtype=torch.float64))
    e_G = gb.U * G.abs() + torch.where((pre.abs() <= fwd_bound) & (m != 0), (d_ts * m).abs(), torch.zeros((), dtype=torch.float64))
    mode = "f32" if ops.precision() == "f32" else "f16x3"
    e_hat = lambda h: kb.MARGIN["normalize"] * gb.U * h.abs() * (kb.cs(C) + 4)   # noqa: E731
    bounds = {}
    for key, Gm, eGm, h, tok in (("src", G.transpose(1, 2), e_G.transpose(1, 2), qh, ts), ("tar", G, e_G, xh, tt)):
        s = 2.0 ** (eb.weight_exponent(G) if mode != "f32" else 0)                  # the range normalisation: a power of two, undone exactly
        _, e_prod = eb.reference("bmm_nn", (Gm * s).float(), h.float(), mode, b_fmt="act", device="cpu")
        e_dn = e_prod / s + eGm @ h.abs() + Gm.abs() @ e_hat(h)
        dn = Gm @ h
        rows = tok[:, 1:].reshape(B * P, C)
        _, nb = kb.reference("normalize_bwd", dict(rows=B * P, n=C), dict(x=rows, dq=dn.reshape(B * P, C)))
        hh, nrm = F.normalize(rows.double(), dim=1), rows.double().norm(dim=1, keepdim=True)
        e = e_dn.reshape(B * P, C)
        bounds[key] = (nb + (e + hh.abs() * (hh.abs() * e).sum(1, keepdim=True)) / nrm).view(B, P, C)

    x, q = ts.cuda().requires_grad_(True), tt.cuda().requires_grad_(True)
    ag.similarity_volume(x, q, mask.cuda()).backward(dout.cuda())
    for key, got, ref in (("src", x.grad, a.grad), ("tar", q.grad, b.grad)):
        got = got.cpu()
        assert bool((got[:, 0] == 0).all()), "the cls row takes no gradient"
        for lo, hi in ((0, 32), (32, 33)):           # the images under the adjoint's grid cap and the one beyond it
            eb.check(f"similarity_volume adjoint d{key} images {lo}..{hi - 1}", got[lo:hi, 1:], ref[lo:hi, 1:], bounds[key][lo:hi], "simvol_autograd")
    print(f"[worst] simvol_autograd: {eb.WORST['simvol_autograd'][0]:.3g} at {eb.WORST['simvol_autograd'][1]}")


@gpu
def test_pose_kernels_treat_every_item_on_its_own():
    """Row b of a batched pp_calc_pred_Ms / pp_pose_recovery_2d call is bit-equal to the same item run alone (B = 1), across the
    64-thread block boundary; a NaN planted in one item's inputs appears in that item's output only."""
    B = 130
    inp = gb.pose_inputs(B, "dense", seed=3)
    full_ms, full_pose = run_hip("pred_ms", inp), run_hip("pose2d", inp)
    for b in (0, 63, 64, 65, 129):
        one = {k: (v[b:b + 1].clone() if torch.is_tensor(v) else v) for k, v in inp.items()}
        assert torch.equal(run_hip("pred_ms", one)[0], full_ms[b]), b
        assert torch.equal(run_hip("pose2d", one)[0], full_pose[b]), b
    for b, key, col in ((64, "tem_K", 0), (63, "tem_pose", 3), (129, "tem_M", 0)):      # (tem_pose: the translation, which both kernels read)
        bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in inp.items()}
        bad[key][b, 0, col] = float("nan")
        others = torch.arange(B) != b
        for op, full in (("pred_ms", full_ms), ("pose2d", full_pose)):
            got = run_hip(op, bad)
            assert torch.equal(got[others], full[others]), (op, key, b)
            assert bool(torch.isnan(got[b]).any()), (op, key, b)


@gpu
def test_identity_affine_gives_exactly_half_a_patch_at_every_mask_size():
    """pred_Ms = I and a mask of ones: the patch centre over the patch size less the grid index is exactly 0.5, at every size."""
    from picopose_amd.utils.correspondence import compute_init_correspondences

    for size in (16, 32, 224, 448):
        f, c = compute_init_correspondences(torch.eye(3).repeat(2, 1, 1).cuda(), torch.ones(2, size, size).cuda())
        assert bool((f == 0.5).all()) and bool((c == 1).all()), size
