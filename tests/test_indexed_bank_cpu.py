"""CPU: the indexed-bank entries (pp_stage1_*_indexed, matching_templates_indexed) reject bad arguments before any launch.
No GPU here: every call below returns (or raises) before it would touch the device."""
import ctypes

import pytest
import torch

from picopose_amd import _lib
from picopose_amd.utils import matching as hm

PP_EINVAL, PP_EWORKSPACE = -1, -2


def _aligned(buf, a):
    p = ctypes.addressof(buf)
    return p + (-p) % a


def test_indexed_workspace_query():
    L = _lib.lib()
    need, plain = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.pp_stage1_indexed_workspace_bytes(32, 162, 768, ctypes.byref(need)) == 0
    assert L.pp_stage1_workspace_bytes(32, 162, 768, ctypes.byref(plain)) == 0
    assert plain.value < need.value <= plain.value + 4096        # the grouping: (B + 1) walk entries and B objects
    assert L.pp_stage1_indexed_workspace_bytes(0, 162, 768, ctypes.byref(need)) == PP_EINVAL
    assert L.pp_stage1_indexed_workspace_bytes(32, 0, 768, ctypes.byref(need)) == PP_EINVAL
    assert L.pp_stage1_indexed_workspace_bytes(32, 162, 768, None) == PP_EINVAL


def test_indexed_abi_rejects_bad_arguments():
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p16, ws = _aligned(buf, 16), _aligned(buf, 256)
    B, N, C, k = 4, 8, 64, 2
    need = ctypes.c_size_t()
    assert L.pp_stage1_indexed_workspace_bytes(B, N, C, ctypes.byref(need)) == 0

    def scores(idx=p16, n_obj=2, B=B, N=N, C=C, ws=ws, ws_bytes=need.value):
        return L.pp_stage1_scores_indexed(p16, _lib.PP_BANK_F32, idx, n_obj, p16, p16, 224, 224, B, N, C, _lib.PP_MATCH_FAST, 0.0,
                                          ws, ws_bytes, p16, None, None)

    def match(idx=p16, n_obj=2, B=B, N=N, C=C, k=k, ws=ws, ws_bytes=need.value):
        return L.pp_stage1_match_indexed(p16, _lib.PP_BANK_F16, idx, n_obj, p16, p16, 224, 224, B, N, C, k, _lib.PP_MATCH_EXACT,
                                         0.0, ws, ws_bytes, p16, p16, p16, None, None)

    for call in (scores, match):
        assert call(idx=None) == PP_EINVAL                       # null index
        assert call(n_obj=0) == PP_EINVAL                        # n_obj < 1
        assert call(n_obj=-3) == PP_EINVAL
        assert call(n_obj=(1 << 23) // N) == PP_EINVAL           # n_obj * N beyond the bank's row range
        assert call(B=0) == PP_EINVAL                            # bad B, N, C
        assert call(N=0) == PP_EINVAL
        assert call(C=100) == PP_EINVAL
        assert call(C=4096) == PP_EINVAL
        assert call(ws_bytes=need.value - 1) == PP_EWORKSPACE   # workspace too small for the grouping
        assert call(ws=ws + 16) == PP_EWORKSPACE                 # misaligned workspace
    assert match(k=0) == PP_EINVAL and match(k=N + 1) == PP_EINVAL
    # the gathered entries' workspace is not enough for the indexed form
    plain = ctypes.c_size_t()
    assert L.pp_stage1_workspace_bytes(B, N, C, ctypes.byref(plain)) == 0
    assert scores(ws_bytes=plain.value) == PP_EWORKSPACE


def _args(B=3, O=2, N=4, C=64):
    return torch.zeros(O, N, C, 16, 16), torch.zeros(B, C, 16, 16), torch.zeros(B, 224, 224)


@pytest.mark.parametrize("fn", ["matching", "scores"])
def test_matching_templates_indexed_validates_the_index(fn):
    bank, query, mask = _args()

    def call(idx):
        if fn == "matching":
            return hm.matching_templates_indexed(bank, idx, query, None, mask, topk=2)
        return hm.template_scores_indexed(bank, idx, query, mask)

    for bad in (torch.zeros(3, 1, dtype=torch.int64),           # wrong rank
                torch.tensor(0),
                torch.zeros(3, dtype=torch.int32),              # wrong dtype
                torch.zeros(3, dtype=torch.float32),
                torch.zeros(2, dtype=torch.int64),              # length != B
                torch.tensor([0, 2, 1]),                        # out of range (O = 2), checked on the host
                torch.tensor([0, -1, 1]),
                [0, 1, 1]):                                     # not a tensor
        with pytest.raises(_lib.PicoPoseHipError):
            call(bad)
    # a valid index gets past the index checks and stops at the device check (CPU tensors)
    with pytest.raises(_lib.PicoPoseHipError, match="GPU"):
        call(torch.tensor([1, 0, 1]))


def test_indexed_bank_must_be_5d():
    bank, query, mask = _args()
    with pytest.raises(_lib.PicoPoseHipError):
        hm.matching_templates_indexed(bank[0], torch.tensor([0, 0, 0]), query, None, mask)
