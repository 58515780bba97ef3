"""CPU: the host functions of picopose_amd/masks.py that the other files exercise only through their callers — the run-table layout,
run ends and their inverse, the area from the ends — and the named errors of the size, window and frame checks.  The codec's own tests
are in test_test_batch_cpu.py and test_scene_gt_cpu.py, through the names those modules import."""
import numpy as np
import pytest

from picopose_amd import masks

FRAMES = ((1, 1), (5, 7), (1, 130), (130, 1), (48, 64))


def _masks(size):
    """An empty mask, a full one and three random ones of the frame."""
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    return [np.zeros(size, bool), np.ones(size, bool)] + [rng.random(size) < p for p in (0.5, 0.1, 0.9)]


@pytest.mark.parametrize("size", FRAMES)
def test_run_words_layout_and_the_inverse_of_run_ends(size):
    H, W = size
    dense = _masks(size)
    segs = [masks.rle_from_mask(m) for m in dense]
    runs = [masks.run_ends(masks.rle_counts(s, k, "mask", size)) for k, s in enumerate(segs)]
    words, off = masks.run_words(runs)
    n, n_runs = len(runs), sum(len(r) for r in runs)
    assert words.dtype == np.int32 and off.dtype == np.int32 and words.shape == (n_runs + n + 1,) and off.shape == (n + 1,)
    assert off[0] == 0 and off.tolist() == np.concatenate(([0], np.cumsum([len(r) for r in runs]))).tolist()        # exclusive offsets
    assert np.array_equal(words[n_runs:], off) and np.array_equal(words[:n_runs], np.concatenate(runs))               # ends, then offsets
    for k, (m, s, r) in enumerate(zip(dense, segs, runs)):
        ends = words[off[k]:off[k + 1]]
        assert r.dtype == np.int64 and np.array_equal(ends, r) and ends[-1] == H * W
        assert np.all(np.diff(ends) >= 0)
        counts = masks.counts_of_ends(ends)
        assert counts.dtype == np.int64 and counts.tolist() == s["counts"]
        assert masks.area_of_ends(ends) == int(m.sum()) == masks.rle_area_extent(masks.rle_counts(s), H)[0]
        # an odd run index is a run of ones: position x * H + y of the column-major walk is set when an odd number of ends are <= it
        inside = (np.searchsorted(ends, np.arange(H * W), side="right") & 1).astype(bool)
        assert np.array_equal(inside.reshape(W, H).T, m)


def test_a_mask_of_another_size_is_named():
    seg = masks.rle_from_mask(np.ones((5, 7)))
    assert masks.rle_counts(seg, 3, "proposal", (5, 7)).tolist() == [0, 35]
    assert masks.rle_counts(seg, 3, "proposal", [5, 7]).tolist() == [0, 35]
    for size in ((7, 5), (5, 8), (35, 1)):
        with pytest.raises(ValueError, match=r"^proposal 3: mask size \(5, 7\) is not the frame's") as e:
            masks.rle_counts(seg, 3, "proposal", size)
        assert str(size) in str(e.value)
    with pytest.raises(ValueError, match=r"^mask size"):                  # no index: no prefix
        masks.rle_counts(seg, size=(7, 5))
    with pytest.raises(ValueError, match=r"^mask 0: run lengths sum to 34"):          # the codec's own errors carry the same prefix
        masks.rle_counts({"size": [5, 7], "counts": [0, 34]}, 0, "mask", (5, 7))
    with pytest.raises(ValueError, match=r"^detection 2: truncated RLE string"):
        masks.rle_counts({"size": [5, 7], "counts": "d"}, 2)


def test_the_window_check_names_empty_and_outside_windows():
    H, W = 48, 64
    for win in ((0, 48, 0, 64), (47, 48, 63, 64), (3, 9, 5, 6)):
        masks.check_window(win, H, W, 4, "proposal")
    for win in ((5, 5, 0, 4), (6, 5, 0, 4), (0, 4, 7, 7), (0, 4, 9, 7),             # empty
                (-1, 4, 0, 4), (0, 4, -1, 4), (0, 49, 0, 4), (0, 4, 0, 65)):         # leaves the frame
        with pytest.raises(ValueError, match=r"^proposal 4: crop window .* is empty or leaves the 48x64 frame$"):
            masks.check_window(win, H, W, 4, "proposal")
    with pytest.raises(ValueError, match=r"^detection 0: crop window"):
        masks.check_window((0, 0, 0, 0), H, W, 0)


def test_the_frame_check_is_at_two_to_the_31():
    masks.check_frame(1, 1)
    masks.check_frame(2 ** 15, 2 ** 16 - 1)
    masks.check_frame(1, 2 ** 31 - 1)
    for size in ((2 ** 15, 2 ** 16), (1, 2 ** 31), (2 ** 31, 1), (46341, 46341)):
        with pytest.raises(ValueError, match="frame too large for 32-bit pixel indices"):
            masks.check_frame(*size)


def test_one_constant_for_the_mask_limit():
    from picopose_amd import depth_proposals as dp
    from picopose_amd import verify as vf

    assert masks.MAX_MASKS == 4096 and dp.MAX_MASKS is masks.MAX_MASKS and vf.MAX_MASKS is masks.MAX_MASKS
