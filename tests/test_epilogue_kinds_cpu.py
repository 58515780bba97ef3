"""CPU: the switch that forces the pre-split kernel's generic epilogue body (pp_gemm_generic_epilogue) validates its argument and
returns the previous setting — no GPU call."""
from picopose_amd import _lib
from picopose_amd.build import build_lib


def test_generic_epilogue_switch_validates_and_returns_previous():
    build_lib()
    L = _lib.lib()
    assert "pp_gemm_generic_epilogue" in _lib.declared_symbols()
    for bad in (-1, 2, 7):
        assert L.pp_gemm_generic_epilogue(bad) == -1      # PP_EINVAL, setting unchanged
    assert L.pp_gemm_generic_epilogue(0) == 0
    assert L.pp_gemm_generic_epilogue(1) == 0
    assert L.pp_gemm_generic_epilogue(-1) == -1
    assert L.pp_gemm_generic_epilogue(1) == 1
    assert L.pp_gemm_generic_epilogue(0) == 1
    assert L.pp_gemm_generic_epilogue(0) == 0
