"""CPU: the depth proposals (picopose_amd/depth_proposals.py, csrc/pp_depth_proposals.hip) without a GPU — the exported symbols, the
argument checks that precede any device work, and the restatement's own sanity on the scenes the GPU tests use
(tests/depth_proposals_oracle.py): it finds the analytic plane, its component masks are the rectangles exactly, and the tie and
step frames have the properties their tests rely on."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_proposals_oracle as do  # noqa: E402

from picopose_amd import _lib  # noqa: E402
from picopose_amd import depth_proposals as dp  # noqa: E402

ENTRIES = ("pp_depth_plane_workspace_bytes", "pp_depth_plane", "pp_depth_components_workspace_bytes", "pp_depth_components",
           "pp_component_stats_workspace_bytes", "pp_component_stats", "pp_components_rle")


def test_the_library_exports_the_entries_with_argtypes():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in ENTRIES:
        assert name in declared and getattr(L, name).argtypes is not None, name


def test_the_abi_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    need = ctypes.c_size_t()
    buf = (ctypes.c_char * 1024)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256      # an aligned non-null address; never dereferenced by the checks
    assert L.pp_depth_plane_workspace_bytes(2, 480, 640, 256, ctypes.byref(need)) == 0
    assert need.value == 2048 + 48128                               # roundup256(4 * 2 * 256) + roundup256(80 * 2 * 300)
    assert L.pp_depth_plane_workspace_bytes(2, 480, 640, 1025, ctypes.byref(need)) == -1
    assert L.pp_depth_plane_workspace_bytes(1, 65536, 32768, 8, ctypes.byref(need)) == -1           # H W = 2^31
    assert L.pp_depth_plane(None, None, 1, 8, 8, 16, 0, 5.0, 3, None, 0, None, None, None, None) == -1
    assert L.pp_depth_plane(p, p, 1, 8, 8, 0, 0, 5.0, 3, p, 1 << 20, p, p, p, None) == -1            # n_hyp
    assert L.pp_depth_plane(p, p, 1, 8, 8, 16, 0, -1.0, 3, p, 1 << 20, p, p, p, None) == -1          # tau
    assert L.pp_depth_plane(p, p, 1, 8, 8, 16, 0, float("nan"), 3, p, 1 << 20, p, p, p, None) == -1
    assert L.pp_depth_plane(p, p, 1, 8, 8, 16, 0, 5.0, 2, p, 1 << 20, p, p, p, None) == -1           # min_inliers
    assert L.pp_depth_plane(p, p, 1, 8, 8, 16, 0, 5.0, 3, p, 16, p, p, p, None) == -2                # PP_EWORKSPACE: short
    assert L.pp_depth_plane(p, p, 1, 8, 8, 16, 0, 5.0, 3, p + 4, 1 << 20, p, p, p, None) == -2       # ... misaligned
    assert L.pp_depth_components_workspace_bytes(1, 8, 8, ctypes.byref(need)) == 0 and need.value == 0
    assert L.pp_depth_components(None, None, None, None, 1, 8, 8, 10.0, 400.0, 3000.0, 15.0, None, 0, None, None) == -1
    assert L.pp_depth_components(p, p, p, p, 1, 8, 8, 10.0, 400.0, 0.0, 15.0, None, 0, p, None) == -1           # max_range
    assert L.pp_depth_components(p, p, p, p, 1, 8, 8, 10.0, 400.0, 3000.0, -1.0, None, 0, p, None) == -1        # max_step
    assert L.pp_depth_components(p, p, p, p, 1, 8, 8, float("nan"), 400.0, 3000.0, 15.0, None, 0, p, None) == -1
    assert L.pp_depth_components(p, p, p, p, 0, 8, 8, 10.0, 400.0, 3000.0, 15.0, None, 0, p, None) == -1
    assert L.pp_component_stats_workspace_bytes(2, 5, 7, ctypes.byref(need)) == 0 and need.value == 1792        # roundup256(24 * 70)
    assert L.pp_component_stats(None, 1, 8, 8, 1, 64, 0, 4, None, 0, None, None, None) == -1
    assert L.pp_component_stats(p, 1, 8, 8, 0, 64, 0, 4, p, 1 << 20, p, p, None) == -1               # min_area
    assert L.pp_component_stats(p, 1, 8, 8, 9, 8, 0, 4, p, 1 << 20, p, p, None) == -1                # max_area < min_area
    assert L.pp_component_stats(p, 1, 8, 8, 1, 64, 0, 0, p, 1 << 20, p, p, None) == -1               # cap
    assert L.pp_component_stats(p, 1, 8, 8, 1, 64, 0, 4, p, 8, p, p, None) == -2
    I = ctypes.c_int * 6
    ip = ctypes.POINTER(ctypes.c_int)
    sel = lambda *v: ctypes.cast(I(*v), ip)  # noqa: E731
    assert L.pp_components_rle(None, 1, 8, 8, None, None, 1, None, None, 0, None, None, None) == -1
    assert L.pp_components_rle(p, 1, 8, 8, p, sel(0, 0, 0, 0, 7, 7), 1, None, None, 0, None, None, None) == -1  # count pass without n_runs
    assert L.pp_components_rle(p, 1, 8, 8, p, sel(1, 0, 0, 0, 7, 7), 1, None, None, 0, p, None, None) == -1     # image
    assert L.pp_components_rle(p, 1, 8, 8, p, sel(0, 64, 0, 0, 7, 7), 1, None, None, 0, p, None, None) == -1    # root
    assert L.pp_components_rle(p, 1, 8, 8, p, sel(0, 0, 0, 0, 8, 7), 1, None, None, 0, p, None, None) == -1     # box leaves the frame
    assert L.pp_components_rle(p, 1, 8, 8, p, sel(0, 0, 3, 0, 2, 7), 1, None, None, 0, p, None, None) == -1     # empty box
    off = (ctypes.c_int * 2)(0, 5)
    assert L.pp_components_rle(p, 1, 8, 8, p, sel(0, 0, 0, 0, 7, 7), 1, p, ctypes.cast(off, ip), 4, None, p, None) == -1   # offsets do not end in n_runs
    assert L.pp_components_rle(p, 1, 8, 8, p, sel(0, 0, 0, 0, 7, 7), 0, None, None, 0, p, None, None) == -1     # n


def test_the_wrappers_reject_bad_arguments_without_a_gpu():
    depth, cams = torch.zeros((2, 8, 9)), torch.ones((2, 4))
    plane, has = torch.zeros((2, 4)), torch.zeros((2,), dtype=torch.int32)
    labels = torch.zeros((2, 8, 9), dtype=torch.int32)
    bad = [lambda: dp.plane_fit(depth.double(), cams), lambda: dp.plane_fit(depth[0], cams), lambda: dp.plane_fit(depth, cams[:1]),
           lambda: dp.plane_fit(depth, cams, tau=-1.0), lambda: dp.plane_fit(depth, cams, tau=float("inf")), lambda: dp.plane_fit(depth, cams, n_hyp=0),
           lambda: dp.plane_fit(depth, cams, n_hyp=1025), lambda: dp.plane_fit(depth, cams, n_hyp=2.5), lambda: dp.plane_fit(depth, cams, seed=-1),
           lambda: dp.plane_fit(depth, cams, min_inliers=2),
           lambda: dp.components(depth, cams, plane[:1], has), lambda: dp.components(depth, cams, plane, has.long()),
           lambda: dp.components(depth, cams, plane, has, min_height=5.0, max_height=5.0), lambda: dp.components(depth, cams, plane, has, max_range=0.0),
           lambda: dp.components(depth, cams, plane, has, max_step=-0.1), lambda: dp.components(depth, cams, plane, has, max_step=float("nan")),
           lambda: dp.component_stats(labels.float()), lambda: dp.component_stats(labels, min_area=0), lambda: dp.component_stats(labels, min_area=5, max_area=4),
           lambda: dp.component_stats(labels, cap=0),
           lambda: dp.component_rle(labels, np.zeros((0, 6), np.int32)), lambda: dp.component_rle(labels, np.zeros((1, 5), np.int32)),
           lambda: dp.component_rle(labels, np.array([[2, 0, 0, 0, 1, 1]])), lambda: dp.component_rle(labels, np.array([[0, 72, 0, 0, 1, 1]])),
           lambda: dp.component_rle(labels, np.array([[0, 0, 0, 0, 9, 1]])), lambda: dp.component_rle(labels, np.array([[0, 0, 0, 3, 1, 2]])),
           lambda: dp.component_rle(labels, np.array([[0.0, 0, 0, 0, 1, 1]]))]
    d16, K = np.zeros((8, 9), np.uint16), np.eye(3)
    bad += [lambda: dp.depth_proposals(d16, K), lambda: dp.depth_proposals(d16.astype(np.float32), K, depth_scale=1.0),
            lambda: dp.depth_proposals(d16.astype(np.int32), K), lambda: dp.depth_proposals(d16, np.zeros((3, 3)), depth_scale=1.0),
            lambda: dp.depth_proposals(d16, K, depth_scale=1.0, max_area_frac=0.0), lambda: dp.depth_proposals(d16, K, depth_scale=1.0, max_area_frac=1.5),
            lambda: dp.depth_proposals(d16, K, depth_scale=1.0, min_area_px=0), lambda: dp.depth_proposals(d16, K, depth_scale=1.0, min_area_px=60),
            lambda: dp.depth_proposals(d16, K, depth_scale=1.0, min_area_px=5, max_proposals=0),
            lambda: dp.depth_proposals(d16, K, depth_scale=1.0, min_area_px=5, n_hyp=4096),
            lambda: dp.depth_proposals(d16, K, depth_scale=1.0, min_area_px=5, tau=-1.0),
            lambda: dp.depth_proposals(d16, K, depth_scale=1.0, min_area_px=5, min_height=10.0, max_height=5.0),
            lambda: dp.depth_proposals(d16, K, depth_scale=1.0, min_area_px=5, max_step=-1.0)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} was accepted")
    with pytest.raises(_lib.PicoPoseHipError, match="GPU only"):               # good arguments, host tensors: refused, never computed on the CPU
        dp.plane_fit(depth, cams)
    with pytest.raises(_lib.PicoPoseHipError, match="GPU only"):
        dp.depth_proposals(d16, K, depth_scale=1.0, min_area_px=5, device="cpu")


def test_pipeline_routes_the_depth_proposal_keywords():
    from picopose_amd import pipeline

    assert set(pipeline.DEPTH_PROPOSAL_KEYS).isdisjoint(pipeline.LABEL_KEYS + pipeline.LABEL_SHARED_KEYS + pipeline.ASSEMBLE_KEYS)
    with pytest.raises(ValueError, match="one .H, W. image"):
        pipeline.infer_depth_proposals(None, None, np.zeros((1, 4, 4), np.float32), np.eye(3), None, None)
    with pytest.raises(ValueError, match="depth_unit"):
        pipeline.infer_depth_proposals(None, None, np.zeros((4, 4), np.float32), np.eye(3), None, None, depth_unit="m")


def test_the_oracle_finds_the_analytic_plane_and_the_rectangles_exactly():
    """The conditions of the GPU end-to-end test, met by the restatement alone: the winner's consensus is the table (every valid table
    pixel and nothing else), the refit is the scene's plane, and the proposals are the four large rectangles' masks, largest first."""
    depth, cam, masks = do.e2e_scene()
    props, pl, lab = do.proposals(depth, cam, min_inliers=500)
    table = do.valid(depth) & ~np.any(masks, axis=0)
    assert pl["has_plane"] and pl["count"] == pl["refit_count"] == int(table.sum()) and np.array_equal(pl["consensus"], table)
    n = np.array([0.12, -0.42, -0.9])                               # the scene's plane: n . p + 800 = 0, the camera on the positive side
    assert np.abs(pl["plane64"][:3] - n / np.linalg.norm(n)).max() < 1e-6 and abs(pl["plane64"][3] - 800.0) < 1e-3
    big = sorted((m for m in masks if m.sum() >= 200), key=lambda m: -int(m.sum()))
    assert len(big) == 4 and len(props) == 4
    for p, m in zip(props, big):
        assert p["segmentation"] == do.rle_from_mask(m) and p["area"] == int(m.sum())
        ys, xs = np.nonzero(m)
        assert p["bbox"] == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
    assert [p["area"] for p in props] == sorted((p["area"] for p in props), reverse=True) and len({p["area"] for p in props}) == 4
    assert set(np.unique(lab[masks[4]])) == {int(np.flatnonzero(masks[4].ravel())[0])}            # the small one is a component, filtered by area


def test_the_roof_scene_ties_hypotheses_of_both_halves():
    depth, cam = do.roof_scene()
    pl = do.plane(depth, cam, n_hyp=64, min_inliers=100)
    top = np.flatnonzero(pl["scores"] == pl["count"])
    assert len(top) >= 2 and pl["winner"] == top[0]
    W = depth.shape[1]
    side = [{(do.aug_hash(0, 0, 3 * int(h) + k) * depth.size >> 32) % W >= W // 2 for k in range(3)} for h in top]
    assert {True} in side and {False} in side                       # tied winners on either plane: the tie is between different planes


def test_the_label_frames_have_the_properties_their_names_promise():
    for H, W in do.LABEL_SIZES:
        fr = do.label_frames(H, W)
        lab = {k: do.labels(d, do.foreground(d, do.camera(H, W), np.zeros(4, np.float32), False)) for k, d in fr.items()}
        assert (lab["empty"] == -1).all() and (lab["full"] == 0).all()
        assert set(np.unique(lab["serpentine"][lab["serpentine"] >= 0])) == {0}                    # one component, rooted in pixel 0
        cb = lab["checkerboard"]
        assert np.array_equal(cb[cb >= 0], np.flatnonzero(cb.ravel() >= 0))                        # every pixel its own component
        assert lab["last_pixel"][H - 1, W - 1] >= 0 and lab["last_pixel"][0, 0] == 0
        st = lab["steps"]
        roots = [len(np.unique(st[st >= 0]))]
        assert roots[0] == 6, roots                                  # two joined pairs, two split ones
    big = do.big_frame()
    lab = do.labels(big, do.foreground(big, do.camera(480, 640), np.zeros(4, np.float32), False))
    assert set(np.unique(lab[:200][lab[:200] >= 0])) == {0} and (lab[:200] >= 0).sum() == 100 * 640 + 100


def test_run_ends_restate_rle_from_mask():
    m = np.zeros((5, 7), bool)
    m[0, 0] = m[4, 6] = m[2, 3] = True
    lab = np.where(m, 0, -1).astype(np.int32)
    assert do.run_ends(lab, 0).tolist() == [0, 1, 17, 18, 34, 35]
