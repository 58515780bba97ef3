"""COCO run-length masks from a record to the kernel that reads them: the codec, the run tables and the two launches
that read them.  A mask never becomes a dense image on the way; provider/test_batch.py, proposals.py, verify.py, depth_proposals.py and
scene_gt.py share what is here.

COCO run-length encoding (pycocotools' `maskApi.c`, restated; pycocotools is not available to pin it): the (h, w) mask is
walked column by column (Fortran order), so pixel (y, x) is position x * h + y; `counts` alternate a run of 0s and a run of 1s,
starting with a run of 0s that may be empty: an odd run index is a run of ones.  The compressed string stores each count as
little-endian groups of five bits, one character `chr(48 + c)` per group with `c & 0x20` = "another group follows" and bit `0x10` of
the last group sign-extending; from the fourth count on the stored value is the difference to the count two places before.

The run tables (what pp_detections_crop, pp_rle_pack_bits and pp_components_rle take; include/picopose_hip.h): a mask is its run ENDS,
the inclusive prefix sums of its counts (`run_ends`; the last one is h * w); the ends of a call's n masks are concatenated into one
int32 array, and the n + 1 exclusive offsets of the masks, int32 too, follow them in the same allocation (`run_words`).  A host copy of
the offsets travels along, because the entry points validate it before they launch (`RunTable`)."""
import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .utils.preprocess import CLIP_MEAN, CLIP_STD

MAX_MASKS = _lib.PP_MASK_MAX_N       # the masks of one pp_rle_pack_bits, pp_mask_intersections or pp_components_rle call


def _fail(what, index, msg):
    raise ValueError(f"{what} {index}: {msg}" if index is not None else msg)


def _counts_from_string(s, index=None, what="detection"):
    c = np.frombuffer(s.encode("ascii") if isinstance(s, str) else bytes(s), np.uint8).astype(np.int64) - 48
    if c.size == 0:
        return np.zeros(0, np.int64)
    if c.min() < 0 or c.max() > 63:
        _fail(what, index, "RLE string holds a character outside chr(48) .. chr(111)")
    last = (c & 0x20) == 0                                 # the closing group of each count
    if not last[-1]:
        _fail(what, index, "truncated RLE string (the last count announces another group)")
    ends = np.nonzero(last)[0]
    start = np.concatenate(([0], ends[:-1] + 1))
    k = np.arange(c.size) - np.repeat(start, ends - start + 1)
    if k.max() > 6:
        _fail(what, index, "RLE count beyond 32 bits")
    d = np.add.reduceat((c & 0x1f) << (5 * k), start)
    neg = (c[ends] & 0x10) != 0
    d[neg] -= np.int64(1) << (5 * (k[ends][neg] + 1))      # sign extension of the closing group
    counts = d.copy()                                      # count[m] = d[m] + count[m - 2] for m > 2
    counts[1::2] = np.cumsum(d[1::2])
    counts[2::2] = np.cumsum(d[2::2])
    return counts


def rle_counts(segmentation, index=None, what="detection", size=None):
    """COCO RLE of a CNOS record -> the run lengths as int64: `{"size": [h, w], "counts": ...}` with `counts` a list of ints
    (uncompressed) or a str / bytes (compressed, module docstring).  size: the (H, W) frame the mask must have, when given.
    ValueError (prefixed "<what> <index>: " when `index` is given) for a negative count, a truncated string, counts that do not sum
    to h * w, or a mask of another size."""
    try:
        h, w = (int(v) for v in segmentation["size"])
        raw = segmentation["counts"]
    except (KeyError, TypeError, ValueError):
        _fail(what, index, "segmentation must be {'size': [h, w], 'counts': ...}")
    if h <= 0 or w <= 0:
        _fail(what, index, f"bad mask size {(h, w)}")
    if isinstance(raw, (str, bytes, bytearray)):
        counts = _counts_from_string(raw, index, what)
    else:
        counts = np.asarray(raw, dtype=np.int64).reshape(-1)
    if counts.size and counts.min() < 0:
        _fail(what, index, "negative run length")
    if int(counts.sum()) != h * w:
        _fail(what, index, f"run lengths sum to {int(counts.sum())}, the mask has {h} x {w} = {h * w} pixels")
    if size is not None and (h, w) != tuple(size):
        _fail(what, index, f"mask size {(h, w)} is not the frame's {tuple(size)}")
    return counts


def rle_area_extent(counts, h):
    """From the runs alone, in O(runs): (pixel count, (rmin, rmax, cmin, cmax)) of the mask, the extent inclusive as
    np.where(np.any(mask, axis))[0][[0, -1]] gives it, None for an empty mask.  A 1-run [s, e] (inclusive column-major
    indices) covers columns s // h .. e // h, and rows s % h .. e % h if it stays in one column, else all of them."""
    counts = np.asarray(counts, np.int64)
    ends = np.cumsum(counts)
    ones = counts[1::2]
    keep = ones > 0
    area = int(ones.sum())
    if area == 0:
        return 0, None
    s = ends[0::2][:ones.size][keep]
    e = ends[1::2][keep] - 1
    cs, ce = s // h, e // h
    if np.any(cs != ce):
        rmin, rmax = 0, h - 1
    else:
        rmin, rmax = int((s - cs * h).min()), int((e - ce * h).max())
    return area, (rmin, rmax, int(cs[0]), int(ce[-1]))


def rle_from_mask(mask):
    """(H, W) mask (non-zero = set) -> {"size": [H, W], "counts": [...]}: UNCOMPRESSED COCO run lengths, column-major, the first run
    zeros (0 when the first pixel is set) — what `rle_counts` decodes.  numpy on the host."""
    m = mask.cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    if m.ndim != 2 or 0 in m.shape:
        raise ValueError(f"mask must be a non-empty (H, W) array, got shape {m.shape}")
    flat = (m != 0).ravel(order="F")
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    runs = np.diff(np.concatenate(([0], change, [flat.size])))
    if flat[0]:
        runs = np.concatenate(([0], runs))
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": [int(r) for r in runs]}


def check_frame(H, W):
    """The positions x * H + y of a frame are 32-bit on the device."""
    if H * W >= 2 ** 31:
        raise ValueError("frame too large for 32-bit pixel indices")


def check_window(win, H, W, index, what="detection"):
    """A crop window (y1, y2, x1, x2) must hold a pixel and lie in the (H, W) frame; ValueError names the mask."""
    y1, y2, x1, x2 = win
    if y2 <= y1 or x2 <= x1 or y1 < 0 or x1 < 0 or y2 > H or x2 > W:
        _fail(what, index, f"crop window {win} is empty or leaves the {H}x{W} frame")


def run_ends(counts):
    """Run lengths -> the cumulative run ends (int64); the last one is the mask's pixel count h * w."""
    return np.cumsum(np.asarray(counts, np.int64))


def counts_of_ends(ends):
    """The inverse of `run_ends` (int64)."""
    return np.diff(np.concatenate(([0], np.asarray(ends, np.int64))))


def area_of_ends(ends):
    """The set pixels of a mask from its run ends: the odd runs."""
    return int(counts_of_ends(ends)[1::2].sum())


def run_words(runs):
    """Per-mask run ends -> (words: int32, the ends of all masks and then the n + 1 exclusive offsets; offset_host: those offsets,
    int32) — the host side of a `RunTable`, apart from the upload so that a caller can splice the words into a larger staging buffer."""
    off = np.zeros(len(runs) + 1, np.int32)
    np.cumsum([len(r) for r in runs], out=off[1:])
    return np.concatenate(list(runs) + [off]).astype(np.int32), off


class RunTable(NamedTuple):
    """The run tables of n masks on the device: `ends` (n_runs,) and `offset` (n + 1,) int32, views of one buffer; `offset_host`, the
    numpy copy of the offsets that the entry points validate; `n_runs` = offset_host[-1]."""
    ends: torch.Tensor
    offset: torch.Tensor
    offset_host: np.ndarray
    n_runs: int

    @classmethod
    def from_words(cls, words, offset_host):
        """Views into a device buffer that starts with `run_words`' layout (it may go on with a caller's own words)."""
        n_runs, n = int(offset_host[-1]), len(offset_host) - 1
        return cls(words[:n_runs], words[n_runs:n_runs + n + 1], offset_host, n_runs)

    @classmethod
    def upload(cls, runs, device):
        """Per-mask run ends (at least one mask) -> the table on `device`: one buffer, one copy."""
        words, off = run_words(runs)
        return cls.from_words(torch.from_numpy(words).to(device), off)

    def pack(self, hw):
        """-> (bits (n, ceil(hw / 32)) int32, area (n,) int32) on the device: ONE pp_rle_pack_bits launch; bit x * H + y of a row is
        pixel (y, x) of that mask, the layout pp_mask_intersections and pp_pose_verify read.  hw = H * W of the masks' frame."""
        n, words, dev = len(self.offset_host) - 1, (hw + 31) // 32, self.ends.device
        bits = torch.empty((n, words), dtype=torch.int32, device=dev)
        area = torch.empty((n,), dtype=torch.int32, device=dev)
        _lib.call("pp_rle_pack_bits", self.ends, self.n_runs, self.offset, self.offset_host, n, hw, words, bits, area)
        return bits, area

    def crop(self, frame_d, window_d, window, S, rgb_mask_flag, out_rgb, out_mask):
        """ONE pp_detections_crop launch: frame_d (H, W, 3) uint8 on the device, the n masks' crop windows (n, 4) int32 = y1, y2, x1, x2
        on the device (`window_d`) and on the host (`window`, which the entry validates) -> out_rgb (n, 3, S, S) and out_mask (n, S, S)
        float32 (any leading 1), resized and CLIP-normalised, on the current stream."""
        H, W = frame_d.shape[:2]
        mean, std = (ctypes.c_double * 3)(*CLIP_MEAN), (ctypes.c_double * 3)(*CLIP_STD)
        _lib.call("pp_detections_crop", frame_d, H, W, self.ends, self.n_runs, self.offset, window_d, self.offset_host, window,
                  len(window), S, int(rgb_mask_flag), mean, std, out_rgb, out_mask)
