"""CPU: the exact-mode fallback of the evaluator (pipeline.py on_saturation="exact") — its ABI entry, the per-model arithmetic mode and the
fallback walk of infer_image driven by a fake network, an injected PnP and a fake saturation snapshot.  No GPU."""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from netcfg import small_cfg  # noqa: E402

from picopose_amd import _lib, ops  # noqa: E402
from picopose_amd import pipeline  # noqa: E402
from picopose_amd.build import LIB, build_lib  # noqa: E402


def test_saturation_take_is_declared_exported_and_rejects_null_pointers():
    assert "pp_saturation_take" in _lib.declared_symbols()
    build_lib()
    assert hasattr(ctypes.CDLL(LIB), "pp_saturation_take")
    L = _lib.lib()
    word = ctypes.c_uint(0)
    assert L.pp_saturation_take(None, None, None) == -1                  # PP_EINVAL, before any HIP call
    assert L.pp_saturation_take(ctypes.addressof(word), None, None) == -1
    assert L.pp_saturation_take(None, ctypes.addressof(word), None) == -1


def test_net_precision_validates_and_scopes_only_its_own_calls():
    from picopose_amd.picopose import Net

    net = Net(small_cfg())
    assert net.precision is None and net.range_fallbacks == 0
    for mode in ("f32", "f16x3", "f16", None):
        net.precision = mode
        assert net.precision == mode
    for bad in ("fp32", "bf16", "exact", 32):
        with pytest.raises(ValueError):
            net.precision = bad
    assert net.precision is None
    assert "_precision" not in net.state_dict()
    with pytest.raises(ValueError):
        with ops.precision_scope("tf32"):
            pass


def test_precision_scope_is_thread_local_and_leaves_the_global_alone(monkeypatch):
    monkeypatch.setattr(ops, "PRECISION", "f16x3")
    seen = {}
    with ops.precision_scope("f32"):
        assert ops.precision() == "f32" and ops.terms() == 0 and not ops.presplit()
        with ops.precision_scope("f16"):
            assert ops.precision() == "f16" and ops.terms() == 1
        with ops.precision_scope(None):
            assert ops.precision() == "f32"
        assert ops.precision() == "f32"
        t = threading.Thread(target=lambda: seen.setdefault("other", ops.precision()))
        t.start()
        t.join()
        assert ops.PRECISION == "f16x3"
    assert seen["other"] == "f16x3" and ops.precision() == "f16x3" and ops.terms() == 2
    ops.PRECISION = "f32"                     # the global still switches every model that follows it
    assert ops.precision() == "f32"


class _FakeNet:
    """Net's evaluator-facing surface: `net(end_points, hyp)` -> hyp dicts with (B,4,4) stage-2 poses.  Pose t = (instance, exact?, k)."""

    def __init__(self):
        self.precision, self.match_mode, self.range_fallbacks, self._query_stash = None, None, 0, None
        self.calls = []

    def __call__(self, end_points, hyp=5, next_real_rgb=None):
        assert next_real_rgb is None
        ids = end_points["real_rgb"][:, 0, 0, 0].long()
        exact = self.precision == "f32" and self.match_mode == "exact"
        self.calls.append((ids.tolist(), exact))
        outs = []
        for k in range(hyp):
            p = torch.eye(4).repeat(len(ids), 1, 1)
            p[:, 0, 3], p[:, 1, 3], p[:, 2, 3] = ids.float(), float(exact), float(k)
            outs.append({"pred_poses": p})
        return outs


def _data(n):
    rgb = torch.arange(n, dtype=torch.float32).view(1, n, 1, 1, 1).expand(1, n, 3, 2, 2).contiguous()
    return {"real_rgb": rgb, "real_K": torch.eye(3).repeat(1, n, 1, 1), "score": torch.ones(1, n),
            "obj_idx": torch.zeros(1, n, dtype=torch.long)}


def _pnp_fail(outputs, real_K):
    """PnP fails everywhere (stage-2 poses kept) with ratio (hyp - k) / 10: the ranking keeps the hypotheses in order."""
    hyp, B = len(outputs), outputs[0]["pred_poses"].shape[0]
    ratio = np.repeat((hyp - np.arange(hyp, dtype=np.float64))[:, None] / 10, B, 1)
    return np.zeros((hyp, B, 3, 3)), np.zeros((hyp, B, 3, 1)), ratio, np.zeros((hyp, B), bool)


def test_fallback_branch_reruns_only_the_flagged_mini_batch_and_keeps_instance_order(monkeypatch):
    net = _FakeNet()
    taken = []

    def fake_take(device, slot):         # the forward that ran last clamped an operand iff it held instance 2 in the fast mode
        ids, exact = net.calls[-1]
        slot.fill_(int(2 in ids and not exact))
        taken.append(int(slot[0]))
        return slot

    monkeypatch.setattr(ops, "saturation_word", lambda device=None: None)
    monkeypatch.setattr(ops, "saturation_take", fake_take)
    n, hyp = 5, 3
    preds = pipeline.infer_image(net, _data(n), {"tem_rgb": torch.zeros(1, 2, 3, 2, 2)}, hyp=hyp, bs=2, pnp_fn=_pnp_fail,
                                 on_saturation="exact")
    assert net.calls == [([0, 1], False), ([2, 3], False), ([2, 3], True), ([4], False)]
    assert taken == [0, 1, 0, 0]
    assert net.range_fallbacks == 1 and net.precision is None and net.match_mode is None
    assert len(preds) == n
    for i, p in enumerate(preds):
        assert len(p) == hyp
        assert [h["inliers_ratio"] for h in p] == [(hyp - k) / 10 for k in range(hyp)]
        for k, h in enumerate(p):
            assert np.array_equal(h["t_stage_3"], np.array([i, float(i in (2, 3)), k]) * 1000)


def test_raise_mode_takes_no_snapshot(monkeypatch):
    net = _FakeNet()
    monkeypatch.setattr(ops, "saturation_take", lambda device, slot: pytest.fail("the default mode must not take a snapshot"))
    preds = pipeline.infer_image(net, _data(3), {"tem_rgb": torch.zeros(1, 2, 3, 2, 2)}, hyp=2, bs=2, pnp_fn=_pnp_fail)
    assert len(preds) == 3 and net.range_fallbacks == 0 and all(not exact for _, exact in net.calls)


@pytest.mark.parametrize("bad", ["retry", "f32", None, ""])
def test_on_saturation_rejects_unknown_values(bad):
    net = _FakeNet()
    with pytest.raises(ValueError, match="on_saturation"):
        pipeline.infer_batch(net, {"real_rgb": torch.zeros(1, 3, 2, 2), "real_K": torch.eye(3)[None]}, 2, pnp_fn=_pnp_fail, on_saturation=bad)
    with pytest.raises(ValueError, match="on_saturation"):
        pipeline.infer_image(net, _data(2), {"tem_rgb": torch.zeros(1, 2, 3, 2, 2)}, hyp=2, bs=2, pnp_fn=_pnp_fail, on_saturation=bad)
    assert net.calls == []
