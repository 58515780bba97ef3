"""What detection_eval.py and pose_detection_eval.py share on the host: the group plan, its device table, the call plumbing, the curve of a cell."""
import numpy as np
import torch

from . import _lib

REC_THRS = np.linspace(0, 1, 101)


def first(counts):
    """The exclusive prefix sum: where each group starts on an axis that holds the groups back to back."""
    return np.cumsum(counts) - counts


def check_offsets(n, where, largest=0):
    """The kernels' offsets are 32-bit: ValueError at 2^31 pairs (or `largest`, the records of a side) in one `where` ("call", "chunk")."""
    if max(n, largest) >= 2 ** 31:
        raise ValueError(f"{n} pairs in one {where}: more than 32-bit block offsets hold")


def axis(keys, lists, limit, kind, noun):
    """One side: per group (keys: its printable (image, class)) its int64 input rows, ordered and cut by the caller -> ({first, count}
    (n_groups, 2), the rows back to back).  ValueError names the first group with more than `limit` `noun` (None: no bound)."""
    for k, rows in zip(keys, lists):
        if limit is not None and len(rows) > limit:
            raise ValueError(f"image {k[0]}, {kind} {k[1]}: {len(rows)} {noun}, more than the {limit} of one group")
    n = np.array([len(rows) for rows in lists], np.int64)
    return np.stack([first(n), n], axis=1).reshape(-1, 2), np.concatenate(list(lists) + [np.zeros(0, np.int64)])


def plan_groups(keys, scored, truths, limit, kind, noun):
    """Both sides (`axis`; `limit` bounds a group's ground truths) -> (scored {first, count}, truth {first, count}, the offset of each group's
    row-major scored x truth block, scored rows, truth rows, n_pairs).  The 2^31 guard is the callers': pose's plan_groups, _run_chunk."""
    (s, s_index), (t, t_index) = axis(keys, scored, None, kind, noun), axis(keys, truths, limit, kind, noun)
    blocks = s[:, 1] * t[:, 1]
    return s, t, first(blocks), s_index, t_index, int(blocks.sum())


def group_rows(scored, truth, pair):
    """-> the contiguous (n_groups, 5) int32 table {first, count, first, count, block offset} of pp_det_overlaps, pp_det_match, pp_pose_match."""
    return np.ascontiguousarray(np.concatenate([scored, truth, np.asarray(pair)[:, None]], axis=1), dtype=np.int32)


def require_cuda(device, who):
    if torch.device(device).type != "cuda":
        raise _lib.PicoPoseHipError(f"picopose_amd runs on the GPU only: {who} needs a CUDA(HIP) device")
    return torch.device(device)


def uploader(device):
    """-> up(a, side=False).  side=True is THE RULE OF AN EMPTY SIDE: ONE zero goes up, its output tables get width 1 and are cut after the download."""
    return lambda a, side=False: torch.from_numpy(np.ascontiguousarray(a) if np.size(a) or not side else np.zeros(1, np.asarray(a).dtype)).to(device)


def device_marks(timings):
    """-> (mark(name), finish()): mark before and after a launch records an event pair on the current stream; finish adds each pair's
    device seconds to timings[name] (None: nothing is recorded).  finish WAITS ON THE RECORDED END EVENTS, not on the device."""
    marks = {}

    def mark(name):
        if timings is not None:
            marks.setdefault(name, []).append(torch.cuda.Event(enable_timing=True))
            marks[name][-1].record()

    def finish():
        for name, (start, end) in marks.items():
            end.synchronize()
            timings[name] = timings.get(name, 0.0) + start.elapsed_time(end) * 1e-3

    return mark, finish


def pr_curve(matched, ignored, npig):
    """One cell: matched, ignored (T, n) bool by descending score, npig > 0 non-ignored ground truths -> (precision (T, 101), recall (T,)).
    pr = tp / (tp + fp + spacing(1)), made non-increasing from the right, where rc = tp / npig reaches REC_THRS; recall = rc[-1] or 0."""
    T, n = matched.shape
    tps = np.cumsum(matched & ~ignored, axis=1).astype(np.float64)
    fps = np.cumsum(~matched & ~ignored, axis=1).astype(np.float64)
    rcs = tps / npig
    prs = np.maximum.accumulate((tps / (fps + tps + np.spacing(1)))[:, ::-1], axis=1)[:, ::-1]
    precision = np.zeros((T, 101))
    for t in range(T):
        ind, row = np.searchsorted(rcs[t], REC_THRS, side="left"), precision[t]
        row[ind < n] = prs[t, ind[ind < n]]
    return precision, rcs[:, -1] if n else np.zeros(T)


def mean_valid(x):
    """The mean of the cells > -1, or -1 when there is none."""
    return float(np.mean(x[x > -1])) if (x > -1).any() else -1.0
