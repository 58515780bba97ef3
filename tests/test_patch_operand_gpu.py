"""pp_patch_operand: the patch embedding's operand written straight from the image bank, bit for bit against the chain it replaces
(gather_rows -> torch.cat -> to_nhwc(c_pad=8) -> split_activation), in both operand formats; its out-of-range rows, its saturation report
and the arguments it rejects."""
import ctypes

import pytest
import torch

gpu = pytest.mark.gpu
PP_OK, PP_EINVAL = 0, -1


def _chain(ops, bank, idx, front):
    """Today's four calls -> the fp16 operand buffer."""
    x = ops.gather_rows(bank, idx) if idx.numel() else bank[:0]
    if front is not None:
        x = torch.cat([front, x])
    img = ops.to_nhwc(x, c_pad=8)
    Bt, H, W, _ = img.shape
    return ops.split_activation(img, Bt, H * W, 8, H * W * 8, 8)


# (O, N, H, W, index, images in front): 2 x 3 images of 28 x 28 (2 x 2 patches; one part-filled tile) with a repeated row, the first row
# and the last row; no selected row at all; the real 224 x 224 row pitch (49 full tiles); two tiles, the second part-filled; a plane
# that is no multiple of 4 floats (the scalar loads)
CASES = [
    (2, 3, 28, 28, [4, 0, 5, 4], 0),
    (2, 3, 28, 28, [4, 0, 5, 4], 1),
    (2, 3, 28, 28, [], 1),
    (1, 2, 224, 224, [1, 0], 1),
    (1, 3, 36, 36, [2, 2, 0], 2),
    (1, 3, 7, 7, [1, 2], 1),
]


@gpu
@pytest.mark.parametrize("mode", ["f16x3", "f16"])
@pytest.mark.parametrize("O,N,H,W,index,nf", CASES)
def test_patch_operand_equals_the_four_call_chain(O, N, H, W, index, nf, mode):
    from picopose_amd import ops

    g = torch.Generator().manual_seed(3)
    tem = torch.randn(O, N, 3, H, W, generator=g).cuda()
    front = torch.randn(nf, 3, H, W, generator=g).cuda() if nf else None
    idx = torch.tensor(index, dtype=torch.int64, device="cuda")
    bank = tem.flatten(0, 1)
    with ops.precision_scope(mode):
        want = _chain(ops, bank, idx, front)
        sp = ops.patch_operand(bank, idx, front=front)
    t = 2 if mode == "f16x3" else 1
    assert sp.terms == t and sp.image == (nf + len(index), H, W) and sp.hl.shape == ((nf + len(index)) * H * W, 8 * t)
    assert torch.equal(sp.hl.view(torch.int16), want.view(torch.int16))
    assert not ops.saturation_raised()


@gpu
def test_an_index_outside_the_bank_is_treated_as_gather_rows_treats_it():
    from picopose_amd import _lib, ops

    H = W = 28
    bank = torch.randn(4, 3, H, W, generator=torch.Generator().manual_seed(4)).cuda()
    idx = torch.tensor([4, 1, -1], dtype=torch.int64, device="cuda")
    L = _lib.lib()
    dst = torch.full((3, 3, H, W), -7.5, device="cuda")
    r_gather = L.pp_gather_rows(bank.data_ptr(), idx.data_ptr(), 4, 3 * H * W, 3, dst.data_ptr(), _lib.stream_ptr())
    out = torch.full((3 * H * W, 16), 3.0, dtype=torch.float16, device="cuda")
    r_patch = L.pp_patch_operand(bank.data_ptr(), 4, idx.data_ptr(), 3, None, 0, H, W, out.data_ptr(), 2, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r_gather == r_patch == PP_OK
    # both leave the rows of an out-of-range index as they were and serve the others
    assert bool((dst[0] == -7.5).all()) and bool((dst[2] == -7.5).all()) and torch.equal(dst[1], bank[1])
    got = out.view(3, H * W, 16)
    assert bool((got[0] == 3.0).all()) and bool((got[2] == 3.0).all())
    want = ops.patch_operand(bank, idx[1:2])
    assert torch.equal(got[1].view(torch.int16), want.hl.view(torch.int16))


@gpu
@pytest.mark.parametrize("mode", ["f16x3", "f16"])
def test_a_value_beyond_the_operand_range_sets_the_saturation_word(mode):
    from picopose_amd import ops

    ops.saturation_raised()
    bank = torch.randn(2, 3, 28, 28, generator=torch.Generator().manual_seed(5)).cuda()
    idx = torch.tensor([1, 0], dtype=torch.int64, device="cuda")
    with ops.precision_scope(mode):
        ops.patch_operand(bank, idx)
        assert not ops.saturation_raised()
        bank[1, 2, 27, 27] = 20000.0              # 4 x 20 000 > 65 504: the last pixel of a plane
        want = _chain(ops, bank, idx, None)
        assert ops.saturation_raised()            # the chain's split pass reports it ...
        sp = ops.patch_operand(bank, idx)
        assert ops.saturation_raised()            # ... and so does the one kernel, with the same clamped terms
    assert torch.equal(sp.hl.view(torch.int16), want.view(torch.int16))


def test_patch_operand_is_declared_and_rejects_bad_arguments():
    """Null and misaligned pointers and inconsistent sizes give PP_EINVAL before any HIP call: no GPU needed."""
    from picopose_amd import _lib

    assert "pp_patch_operand" in _lib.declared_symbols() and "pp_flow_operand" in _lib.declared_symbols()
    L = _lib.lib()
    a = (ctypes.c_float * 64)()
    p = (ctypes.addressof(a) + 15) // 16 * 16
    good = dict(bank=p, rows=6, index=p, n=4, front=p, nf=1, H=28, W=28, out=p, terms=2)
    call = lambda **kw: L.pp_patch_operand(*{**good, **kw}.values(), None)  # noqa: E731
    for name in ("bank", "index", "front", "out"):
        assert call(**{name: None}) == PP_EINVAL, name
    for name in ("bank", "front", "out"):
        assert call(**{name: p + 4}) == PP_EINVAL, name          # 16-byte accesses on every side
    for name, bad in (("rows", 0), ("n", -1), ("nf", -1), ("H", 0), ("W", -3), ("terms", 0), ("terms", 3), ("n", 65535)):
        assert call(**{name: bad}) == PP_EINVAL, (name, bad)
    assert call(n=0, nf=0) == PP_EINVAL                          # nothing to write
    good = dict(flow=p, ld=2, rows=10, out8=p, terms=2)
    call = lambda **kw: L.pp_flow_operand(*{**good, **kw}.values(), None)  # noqa: E731
    for kw in (dict(flow=None), dict(out8=None), dict(out8=p + 8), dict(ld=1), dict(rows=0), dict(terms=0), dict(terms=3)):
        assert call(**kw) == PP_EINVAL, kw
