"""CPU: the C-ABI library builds, loads and exports every symbol include/picopose_hip.h declares.
No compute calls here (no GPU)."""
import ctypes

import pytest

from picopose_amd import _lib
from picopose_amd.build import LIB, build_lib


def test_library_exports_every_declared_symbol():
    build_lib()
    lib = ctypes.CDLL(LIB)
    names = _lib.declared_symbols()
    assert "pp_stage1_match" in names and "pp_topk" in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/picopose_hip.h but not exported"


_MINI_HEADER = r'''
/* one prototype per form include/picopose_hip.h uses */
#ifndef MINI_H
#define MINI_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PP_PLAIN 7
#define PP_NEGATIVE (-3) /* parenthesised */
#define PP_FLOAT 1.0f
#define PP_CONTINUED \
    12 /* a trailing comment that itself runs over the line \
          break, as PP_MATCH_FAST's does */
typedef struct PpX {
    int a, b, c;      /* a declarator list */
    const float* p;
    long long s;
    float x, y;
} PpX;
const char* pp_text(int code);
size_t pp_size(long long n, int c);
int pp_none(void);
int pp_empty();
int pp_ints(int32_t* a, const int64_t* b, const float* const* c, unsigned seed, double d, float f);
int pp_voids(const void* in, void* stream, size_t n, size_t* bytes);
int pp_structs(const PpX* in, PpX* out, long long n);
int pp_Spread(const float* a, /* first */
              int n,          /* second */
              /* a line of its own */
              float* out,
              void* stream);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_header_parser_on_every_form_the_header_uses():
    c = ctypes
    protos, structs, consts, streamed = _lib.parse_header(_MINI_HEADER)
    assert streamed == {"pp_Spread"}                 # `void* stream` LAST; pp_voids has one in the middle, which is an argument like any
    X = structs["PpX"]
    assert list(structs) == ["PpX"] and issubclass(X, c.Structure) and X.__name__ == "PpX"
    assert X._fields_ == [("a", c.c_int), ("b", c.c_int), ("c", c.c_int), ("p", c.c_void_p), ("s", c.c_longlong),
                          ("x", c.c_float), ("y", c.c_float)]
    assert c.sizeof(X) == 40 and X.p.offset == 16 and X.s.offset == 24 and X.y.offset == 36
    vp, i32 = c.c_void_p, c.c_int
    assert protos == {
        "pp_text": (c.c_char_p, [i32]),
        "pp_size": (c.c_size_t, [c.c_longlong, i32]),
        "pp_none": (i32, []),
        "pp_empty": (i32, []),
        "pp_ints": (i32, [vp, vp, vp, c.c_uint, c.c_double, c.c_float]),
        "pp_voids": (i32, [vp, vp, c.c_size_t, vp]),
        "pp_structs": (i32, [c.POINTER(X), c.POINTER(X), c.c_longlong]),
        "pp_Spread": (i32, [vp, i32, vp, vp]),
    }
    assert consts == {"PP_PLAIN": 7, "PP_NEGATIVE": -3, "PP_CONTINUED": 12}
    # a type the parser does not know raises and names the function; it never falls back to int
    # (nor, for a type of several words, back to its first word: `unsigned short` is not `unsigned`)
    for bad in ("int pp_bad(short n);", "int pp_bad(const float* a, uint16_t n);", "wchar_t pp_bad(int n);", "unsigned long pp_bad(int);",
                "int pp_bad(unsigned char);", "int pp_bad(unsigned long);", "int pp_bad(unsigned short n);", "unsigned char pp_bad(int n);"):
        with pytest.raises(ValueError, match="pp_bad"):
            _lib.parse_header(_MINI_HEADER + bad)
    for bad in ("short a;", "unsigned short a;", "unsigned char a; int b;", "long a;"):
        with pytest.raises(ValueError, match="PpY"):
            _lib.parse_header("typedef struct PpY { %s } PpY;" % bad)
    # unnamed parameters of known types still bind
    assert _lib.parse_header("int pp_f(unsigned, long long, unsigned int, const float*);")[0]["pp_f"][1] == [c.c_uint, c.c_longlong, c.c_uint, vp]


def test_declared_symbols_are_the_headers_prototypes():
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "picopose_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counted = re.findall(r"\bpp_[A-Za-z0-9_]+\s*\(", text)         # (letters of either case: pp_calc_pred_Ms; not the PP_E* (-n) macros)
    names = _lib.declared_symbols()
    assert "pp_calc_pred_Ms" in names and "pp_version" in names
    assert names == sorted(names) and len(names) == len(counted) == len(set(counted))


def test_structs_and_constants_of_the_real_header():
    c = ctypes
    assert c.sizeof(_lib.PpAdamStep) == 40 and c.sizeof(_lib.PpAdamTensor) == 48
    assert len(_lib.PpScene._fields_) == 26 and len(_lib.PpGemmDesc._fields_) == 53
    for cls in (_lib.PpGemmDesc, _lib.PpScene, _lib.PpAdamTensor, _lib.PpAdamStep):
        assert cls.__module__ == "picopose_amd._lib" and issubclass(cls, c.Structure)
    assert [n for n, _ in _lib.PpAdamTensor._fields_] == ["p", "m", "v", "hl", "scale2", "n"]
    assert (_lib.PpGemmDesc.M.offset, _lib.PpGemmDesc.a_bs0.offset, _lib.PpScene.n_objects.offset, _lib.PpScene.near.offset) == (56, 96, 160, 180)
    # the values the Python modules used to restate by hand: this list is the test's own statement of them
    old = dict(PP_OK=0, PP_EINVAL=-1, PP_EWORKSPACE=-2, PP_ELAUNCH=-3, PP_MATCH_EXACT=0, PP_MATCH_FAST=1, PP_BANK_F32=0, PP_BANK_F16=1,
               PP_EVAL_MSSD=1, PP_EVAL_MSPD=2, PP_EVAL_ADD=4, PP_EVAL_ADDS=8, PP_VSD_MAX_TAUS=16, PP_DEPTH_REFINE_STRIP_ROWS=8,
               PP_DEPTH_REFINE_SUMS=29, PP_DEPTH_REFINE_MAX_ITERATIONS=1000, PP_MASK_MAX_N=4096, PP_DET_TILE=8, PP_DET_MAX_GT=4096,
               PP_PLANE_MAX_HYP=1024, PP_SYNTH_BG_WORDS=4, PP_SYNTH_TILE=1024)
    for name, value in old.items():
        assert getattr(_lib, name) == value, name
    assert not hasattr(_lib, "PP_PLANE_MIN_CROSS2")                  # a float-valued macro is no constant of the binding
    # ... and the module-level names that read them
    from picopose_amd import depth_proposals, depth_refine, detection_eval, evaluation, masks
    from picopose_amd.provider import synth_scenes

    assert evaluation.KINDS == {"mssd": 1, "mspd": 2, "add": 4, "adds": 8} and evaluation.VSD_MAX_TAUS == 16
    assert (depth_refine.STRIP_ROWS, depth_refine.N_SUMS, depth_refine.MAX_ITERATIONS) == (8, 29, 1000)
    assert (masks.MAX_MASKS, detection_eval.TILE, detection_eval.MAX_GT, depth_proposals.MAX_HYP) == (4096, 8, 4096, 1024)
    assert (synth_scenes.BG_WORDS, synth_scenes.TILE) == (4, 1024)


def test_error_strings_and_workspace_query():
    L = _lib.lib()
    assert L.pp_version() >= 100
    assert L.pp_strerror(0) == b"ok"
    for code in (-1, -2, -3):
        assert len(L.pp_strerror(code)) > 5
    need = ctypes.c_size_t()
    assert L.pp_stage1_workspace_bytes(32, 162, 768, ctypes.byref(need)) == 0
    assert 20e6 < need.value < 200e6
    assert L.pp_stage1_workspace_bytes(0, 162, 768, ctypes.byref(need)) == -1  # PP_EINVAL


def test_argument_validation_needs_no_gpu():
    L = _lib.lib()
    # null pointers / unsupported channel count are rejected before any HIP call
    assert L.pp_stage1_scores(None, None, None, 224, 224, 1, 1, 64, 1, 0.0, None, 0, None, None, None) == -1
    assert L.pp_topk(None, 1, 4, 2, None, None, None) == -1
    # the entry points added for the training forward, the narrow predict layers and the operand-side helpers
    assert L.pp_train_keypoints_workspace_bytes(0) == 0 and L.pp_train_keypoints_workspace_bytes(2) > 2 * 4096 * 24
    assert L.pp_train_keypoints(*([None] * 2), 224, 224, *([None] * 2), 480, 640, *([None] * 10), 2, None, None, None, 0, None) == -1
    assert L.pp_batchnorm_train_workspace_bytes(1000, 256) >= 4 * 256 * 16
    assert L.pp_batchnorm_train(None, None, None, 10, 256, 1e-5, 0.1, None, None, 0, None, None, None, None, 0, None) == -1
    assert L.pp_gather_normalize_rows(None, 64, None, 4, 64, 1e-12, None, None) == -1
    assert L.pp_xent_diag_rows(None, 4, 4, 10.0, None, None) == -1
    assert L.pp_flow_loss_blocks() > 0 and L.pp_flow_loss_sums(None, None, None, 2, 16, 16, 400.0, None, None) == -1
    assert L.pp_conv_narrow_hl(None, 256, 1, 64, 64, 256, None, None, 3, 2, None, None, None) == -1
    assert L.pp_conv_narrow_f32(None, 256, 1, 64, 64, 256, None, None, 3, 2, None, None, None) == -1
    assert L.pp_corr_lookup_nhwc_hl(None, 256, None, None, None, 1, None, 1, 64, 64, 256, 3, 2, 2, None, 80, None) == -1
    assert L.pp_hl_patch_columns(None, 2, 2, 10, None, 640, 638, None) == -1
    assert L.pp_sum_slices(None, 32, 160, 1024, None, 3, None, None) == -1
    # round 6: the Winograd F(4x4, 3x3) entries reject null operands, maps that are no multiple of the 4x4 tile, channel counts off
    # the operand's 8-column groups, a tile count above the padded row count and byte extents beyond the 32-bit buffer offsets
    import ctypes as c
    buf = (c.c_char * 64)()
    p = c.addressof(buf) + (-c.addressof(buf)) % 16
    assert L.pp_winograd4_input_hl(None, 64, 64 * 64 * 64, 1, 64, 64, 64, 0, None, 256, None) == -1
    assert L.pp_winograd4_input_hl(p, 64, 62 * 64 * 64, 1, 62, 64, 64, 0, p, 256, None) == -1          # H % 4
    assert L.pp_winograd4_input_hl(p, 60, 64 * 64 * 60, 1, 64, 64, 60, 0, p, 256, None) == -1          # C % 8
    assert L.pp_winograd4_input_hl(p, 64, 64 * 64 * 64, 1, 64, 64, 64, 0, p, 255, None) == -1          # P_pad < tiles
    assert L.pp_winograd4_input_hl(p, 1024, 64 * 64 * 1024, 400, 64, 64, 1024, 0, p, 102400, None) == -1   # operand beyond 4 GiB of offsets
    assert L.pp_winograd4_weight_f32(None, 64, 64, 576, None, None) == -1
    assert L.pp_winograd4_weight_f32(p, 64, 64, 575, p, None) == -1                                    # ldw < 9 Cin
    assert L.pp_winograd4_output(None, 64, 1, 64, 64, 64, None, 0, None, None, None, 64, None, 64, 0, 256, None) == -1
    assert L.pp_winograd4_output(p, 64, 1, 64, 64, 64, None, 0, None, None, None, 64, None, 64, 0, 256, None) == -1   # neither output
    assert L.pp_winograd4_output(p, 64, 1, 64, 64, 64, None, 7, None, None, p, 64, None, 64, 0, 256, None) == -1      # activation code
    assert L.pp_winograd4_output(p, 64, 1, 64, 64, 64, None, 0, p, None, None, 64, p, 64, 0, 256, None) == -1         # residual without fp32 out
    assert L.pp_winograd4_output(p, 32, 1, 64, 64, 64, None, 0, None, None, p, 64, None, 64, 0, 256, None) == -1      # ld_y < Cout
    assert L.pp_winograd4_chain(None, 64, 1, 64, 64, 64, None, 0, 0, None, 256, None) == -1
    assert L.pp_winograd4_chain(p, 64, 1, 64, 48, 64, None, 0, 0, p, 256, None) == -1                  # widths 16 / 32 / 64 only
    assert L.pp_winograd4_chain(p, 48, 1, 64, 64, 48, None, 0, 0, p, 256, None) == -1                  # C % 32
    assert L.pp_winograd_chain_f32(None, 1, 64, 64, 64, None, 0, 0, None, None) == -1
    assert L.pp_winograd_chain_f32(p, 1, 63, 64, 64, None, 0, 0, p, None) == -1                        # H % 2
    assert L.pp_winograd_chain_f32(p, 1, 64, 24, 64, None, 0, 0, p, None) == -1
    # ... the resize with both outputs (channel count off the operand's 8-column groups, a missing output, operand format other than 1 / 2 terms)
    assert L.pp_resize_bilinear_nhwc_dual(None, 1, 16, 16, 64, 32, 32, 1.0, None, None, 2, None) == -1
    assert L.pp_resize_bilinear_nhwc_dual(p, 1, 16, 16, 60, 32, 32, 1.0, p, p, 2, None) == -1
    assert L.pp_resize_bilinear_nhwc_dual(p, 1, 16, 16, 64, 32, 32, 1.0, None, p, 2, None) == -1
    assert L.pp_resize_bilinear_nhwc_dual(p, 1, 16, 16, 64, 32, 32, 1.0, p, p, 3, None) == -1
    # ... and the correlation lookup's arithmetic argument: PP_PREC_F32 / F16X3 / F16 (0 / 1 / 2), nothing else
    assert L.pp_corr_lookup_nhwc_ex(p, 64, p, None, None, 1, p, 1, 16, 16, 64, 1, 2, 2, 3, p, 32, None) == -1


def _header_text():
    import os

    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "picopose_hip.h")).read()


def test_call_appends_a_stream_exactly_where_the_header_has_one():
    import re

    text = re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S)
    last_is_stream = {m.group(1): re.search(r"(^|,)\s*void\s*\*\s*stream\s*$", m.group(2)) is not None
                      for m in re.finditer(r"\b(pp_\w+)\s*\(([^()]*)\)\s*;", text)}
    assert set(last_is_stream) == set(_lib.declared_symbols())
    assert any(last_is_stream.values()) and not all(last_is_stream.values())
    for name, want in last_is_stream.items():
        if _lib._PROTOTYPES[name][0] is ctypes.c_int:
            assert _lib._plan(name)[2] == want, name
        else:                                        # a size query or pp_strerror: no status, no plan, no stream
            assert not want, name
            with pytest.raises(TypeError, match=name):
                _lib._plan(name)


def test_call_raises_on_a_rejecting_entry():
    import torch

    x, y = torch.zeros(4, 8), torch.zeros(4, 8)
    text = _lib.lib().pp_strerror(_lib.PP_EINVAL).decode()
    for args in ((x, 0, 8, 1e-12, y), (None, 0, 8, 1e-12, None)):        # n = 0: PP_EINVAL before any device work
        with pytest.raises(_lib.PicoPoseHipError) as e:
            _lib.call("pp_descriptor_normalize", *args, stream=None)
        assert "pp_descriptor_normalize" in str(e.value) and text in str(e.value)
        with pytest.raises(_lib.PicoPoseHipError) as e:
            _lib.call("pp_descriptor_normalize", *args, stream=None, what="label")
        assert "label failed" in str(e.value) and text in str(e.value) and "pp_descriptor_normalize" not in str(e.value)


def test_call_converts_like_the_hand_written_spelling():
    import numpy as np

    def size(query, *args):
        need = ctypes.c_size_t()
        _lib.call(query, *args, ctypes.byref(need))
        return need.value

    off = np.array([0, 100, 350, 1000], dtype=np.int32)
    by_hand = ctypes.c_size_t()
    assert _lib.lib().pp_model_diameter_workspace_bytes(off.ctypes.data, 3, ctypes.byref(by_hand)) == _lib.PP_OK and by_hand.value > 0
    assert size("pp_model_diameter_workspace_bytes", off, 3) == by_hand.value
    assert size("pp_model_diameter_workspace_bytes", off.ctypes.data, 3) == by_hand.value
    assert _lib.workspace_bytes("pp_model_diameter_workspace_bytes", off, 3) == by_hand.value
    assert _lib.address(off[1:]) == off.ctypes.data + 4 and _lib.address(None) is None      # a view passes its own address

    tensors = (_lib.PpAdamTensor * 2)()
    for t, n in zip(tensors, (1000, 4096)):
        t.p, t.m, t.v, t.n = 256, 512, 768, n            # (addresses are not read by the size query)
    assert _lib.lib().pp_adam_workspace_bytes(tensors, 2, ctypes.byref(by_hand)) == _lib.PP_OK and by_hand.value > 0
    assert size("pp_adam_workspace_bytes", tensors, 2) == by_hand.value
    assert size("pp_adam_workspace_bytes", ctypes.byref(tensors[0]), 2) == by_hand.value      # (tensors[0] shares the array's memory)
    assert size("pp_adam_workspace_bytes", tensors[0], 1) == size("pp_adam_workspace_bytes", ctypes.byref(tensors[0]), 1) > 0


def test_call_misuse_is_a_type_error_naming_the_entry():
    need = ctypes.c_size_t()
    with pytest.raises(TypeError, match=r"pp_descriptor_normalize takes 5 arguments and a stream, 4 given"):
        _lib.call("pp_descriptor_normalize", None, 0, 8, 1e-12, stream=None)
    with pytest.raises(TypeError, match=r"pp_stage1_workspace_bytes takes 4 arguments, 5 given"):
        _lib.call("pp_stage1_workspace_bytes", 32, 162, 768, ctypes.byref(need), None)
    with pytest.raises(TypeError, match="pp_stage1_workspace_bytes takes no stream"):
        _lib.call("pp_stage1_workspace_bytes", 32, 162, 768, ctypes.byref(need), stream=None)
    for name, args in (("pp_train_keypoints_workspace_bytes", (2,)), ("pp_strerror", (0,))):       # size_t / const char*: not statuses
        with pytest.raises(TypeError, match=name):
            _lib.call(name, *args)


def test_state_dict_names_shapes_equal_the_reference(golden_dir):
    """`Net(cfg).state_dict()` must carry the reference Net's tensors — same names, same ORDER, same shapes and
    dtypes — for ViT-S/B/L, so that Lite.load_from_checkpoint(..., network=model) loads the authors' checkpoint
    (run_test.py:272).  Fixture: tests/golden/state_dict_names.json, dumped from the reference (oracle/gen_golden.py)."""
    import json
    import os
    import types

    from picopose_amd.picopose import Net

    ns = types.SimpleNamespace
    table = json.load(open(os.path.join(golden_dir, "state_dict_names.json")))
    widths = {"dinov2_vits14": (384, [[0, 2], [3, 5], [6, 8], [9, 11]]), "dinov2_vitb14": (768, [[0, 2], [3, 5], [6, 8], [9, 11]]),
              "dinov2_vitl14": (1024, [[0, 5], [6, 11], [12, 17], [18, 23]])}
    assert set(table) == set(widths)
    for vit, (C, idx) in widths.items():
        cfg = ns(hypothesis=5, stage1=ns(vit_type=vit, pretrained=False, interaction_indexes=idx), stage2=ns(in_channel=256, hidden_dim=256),
                 stage3=ns(nclass=1, in_channels=C, use_bn=True, out_channels=[256, 512, 1024, 1024], num_levels=3, radius=4))
        got = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in Net(cfg).state_dict().items()]
        assert got == table[vit], next((a, b) for a, b in zip(got, table[vit]) if a != b)
    assert len(table["dinov2_vitl14"]) == 603


def test_pack_cache_is_dropped_when_a_checkpoint_loads_through_the_top_level_net():
    """nn.Module.load_state_dict never calls a child's load_state_dict, so a pack-once cache keyed on
    nothing survived `Net.load_state_dict` and later forwards mixed old packed conv weights with new linears."""
    import sys
    import os

    import torch

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from netcfg import small_cfg

    from picopose_amd.model.common import Packed
    from picopose_amd.picopose import Net
    from picopose_amd.utils.seeding import seeded_state_dict

    net = Net(small_cfg())
    net.load_state_dict(seeded_state_dict(net.state_dict(), 1))
    packed = [m for m in net.modules() if isinstance(m, Packed)]
    assert len(packed) >= 4
    fd = net.offset_regressor.flow_decoder
    old = fd.packed()["fp0_p"].clone()                       # packs on first use (pure re-layout: runs on the CPU too)
    for m in packed:
        m._pack_cache = m._pack_cache or {"stale": True}
    net.load_state_dict(seeded_state_dict(net.state_dict(), 2))
    assert all(m._pack_cache is None for m in packed)
    assert not torch.equal(fd.packed()["fp0_p"], old)
    # loading through a wrapper one level further up (Lightning's `network.` prefix) drops it as well
    wrapper = torch.nn.Module()
    wrapper.network = net
    fd.packed()
    wrapper.load_state_dict({"network." + k: v for k, v in seeded_state_dict(net.state_dict(), 3).items()})
    assert fd._pack_cache is None


def test_pack_cache_follows_in_place_parameter_updates():
    """the packed / BN-folded copies are derived from the parameters; an in-place update between two forwards
    (an optimizer step, `with torch.no_grad(): p.mul_()`) must not leave them stale.  The cache records every source tensor's
    (address, version) and rebuilds on a mismatch; a BatchNorm buffer update re-folds the eval packing only.
    ADVICE r03: a write through `p.data` moves NEITHER number (`.data` is a view with its own version counter) — that case is
    the caller's: `Net.invalidate_packed()` after it.  Both behaviours are pinned here."""
    import os
    import sys

    import torch

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from netcfg import small_cfg

    from picopose_amd.picopose import Net
    from picopose_amd.utils.seeding import seeded_state_dict

    net = Net(small_cfg())
    net.load_state_dict(seeded_state_dict(net.state_dict(), 1))
    fd = net.offset_regressor.flow_decoder
    first = fd.packed()
    assert fd.packed() is first                                              # unchanged sources: the cache is reused
    old = first["proj0"].clone()
    with torch.no_grad():
        getattr(fd.proj[0], "0").weight.mul_(2.0)                                       # an optimizer-style in-place step
    assert not torch.equal(fd.packed()["proj0"], old)
    second = fd.packed()
    with torch.no_grad():
        getattr(fd.proj[0], "1").running_var.add_(1.0)                                  # a BatchNorm buffer moved: the fold is stale
    third = fd.packed()
    assert third is not second and not torch.equal(third["proj0"], second["proj0"])
    fd.invalidate_packed()
    assert fd._pack_cache is None and torch.equal(fd.packed()["proj0"], third["proj0"])
    # a write through .data: invisible to (address, version) — documented — and picked up after Net.invalidate_packed()
    w = getattr(fd.proj[0], "0").weight
    v0, a0 = w._version, w.data_ptr()
    w.data.mul_(0.5)
    assert (w._version, w.data_ptr()) == (v0, a0)
    assert torch.equal(fd.packed()["proj0"], third["proj0"])                  # stale, as documented
    net.invalidate_packed()
    assert all(m._pack_cache is None for m in net.modules() if hasattr(m, "_pack_cache"))
    assert not torch.equal(fd.packed()["proj0"], third["proj0"])


@pytest.mark.gpu
def test_call_passes_a_views_address_and_launches_on_the_current_stream():
    import torch

    x = torch.randn(3, 8, generator=torch.Generator().manual_seed(0)).cuda()
    ref = torch.nn.functional.normalize(x.double(), dim=1)
    tol = 8 * 2.0 ** -24                 # unit rows from an 8-term fp32 sum of squares, a square root and a division
    y = torch.zeros_like(x)
    _lib.call("pp_normalize_rows", x, 3, 8, 1e-12, y)
    torch.cuda.synchronize()
    assert (y.double() - ref).abs().max().item() <= tol
    y = torch.zeros(2, 8, device="cuda")
    _lib.call("pp_normalize_rows", x[1:], 2, 8, 1e-12, y)          # a view is passed as ITS address, not its storage's
    torch.cuda.synchronize()
    assert (y.double() - ref[1:]).abs().max().item() <= tol
    # the current stream is the one used: the input is produced on a side stream and only that stream is waited for
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.randn(1 << 22, device="cuda").sort().values           # work ahead of the launch on the same stream
        x2 = x + big[:1] * 0
        y2 = torch.zeros_like(x)
        _lib.call("pp_normalize_rows", x2, 3, 8, 1e-12, y2)
    side.synchronize()
    assert (y2.double() - ref).abs().max().item() <= tol


@pytest.mark.gpu
def test_library_loaded_before_torch_still_launches():
    """`__graft_entry__.build()` opens the library before anything has imported torch.  PyTorch-ROCm bundles its own HIP
    runtime; if the library bound to /opt/rocm's copy instead, the process would hold two runtimes and every launch on a
    torch stream would fail (seen on the GPU box: build() followed by smoke() in one process).  _lib.lib() therefore
    imports torch first — checked here in a fresh interpreter."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import __graft_entry__ as g; g.build(); import torch; from picopose_amd.utils import matching as hm; "
            "g0 = torch.Generator().manual_seed(0); bank = torch.randn(1, 4, 384, 16, 16, generator=g0).cuda(); "
            "q = torch.randn(1, 384, 16, 16, generator=g0).cuda(); s, i = hm.matching_templates(bank, q, None, torch.ones(1, 224, 224).cuda(), topk=4); "
            "torch.cuda.synchronize(); print('LAUNCH OK', i.tolist())")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and "LAUNCH OK" in r.stdout.decode(), r.stdout.decode()[-2000:]
