"""Numpy restatement of the segmented acquisition (include/demod.h, "segmented
acquisition"): the reference of tests/test_acquire_segments_cpu.py and
tests/test_gpu_acquire_segments.py.

Segment s of a batch sym[Wb], P[Wb][K] is windows first[s] .. first[s] +
count[s] - 1 and is acquired as a batch of its own by acquire_ref.acquire on
the slice, after

  the clamp        first' = min(first, Wb), count' = min(count, Wb - first');
  the short rule   count' < R: phases R, phase 0, per_phase 0, metric all 0,
                   sync_window -1, sync_errors 0, first_window count', n_out =
                   n_written = 0, no output;
  the tile budget  (budget given) a segment of count' >= R windows has
                   ceil(count' / tile) tiles; segment s is acquired when the
                   tiles of segments 0 .. s together are <= budget, else it is
                   reported as a short segment is.
"""
import numpy as np

import acquire_ref

TILE = 1024   # DEMOD_ACQUIRE_TILE


def short_result(R, count):
    return dict(metric=np.zeros(R, np.float64), phases=R, phase=0, per_phase=0, sync_window=-1,
                sync_errors=0, reserved=0, first_window=int(count), n_out=0, n_written=0)


def clamp(first, count, Wb):
    """(first', count') as Python ints."""
    f = min(int(first), Wb)
    return f, min(int(count), Wb - f)


def budget_for(max_segments, max_windows, tile=TILE):
    """The tiles demod_acquire_segments_workspace_size(cfg, max_segments,
    max_windows) holds."""
    return -(-int(max_windows) // tile) + int(max_segments)


def acquire_segments(sym, P, R, first, count, sync=(), max_errors=0, cap=None, budget=None, tile=TILE):
    """[(out, result dict)] per segment; out and the dict as acquire_ref.acquire
    gives them on the slice (window indices relative to first')."""
    sym = np.asarray(sym, np.uint8).reshape(-1)
    P = np.asarray(P)
    Wb = sym.size
    assert len(first) == len(count)
    res, used = [], 0
    for f, c in zip(first, count):
        f, c = clamp(f, c, Wb)
        tiles = -(-c // tile) if c >= R else 0
        used += tiles
        if tiles == 0 or (budget is not None and used > budget):
            res.append((np.zeros(0, np.uint8), short_result(R, c)))
        else:
            res.append(acquire_ref.acquire(sym[f:f + c], P[f:f + c], R, sync, max_errors, cap))
    return res


# ---- the slip scenario (a dropped buffer: samples deleted in mid-stream) ------

def slip_drops(n, hop):
    """Samples deleted: hop, 2 hop (hop when R = 2) and (R - 1) hop."""
    R = n // hop
    return sorted({hop, hop if R == 2 else 2 * hop, (R - 1) * hop})


def whole_batch_misreads(stream, truth, ns):
    """Symbols after the slip that a whole-batch acquisition's symbol-rate
    stream (one phase for the whole batch, stream[i] taken for symbol i) gets
    wrong: stream[i] against truth[i] for ns // 2 < i < len(stream)."""
    a = np.asarray(stream)[ns // 2 + 1:]
    b = np.asarray(truth)[ns // 2 + 1:]
    m = min(len(a), len(b))
    return int(np.count_nonzero(a[:m] != b[:m]))


def slip_stream(O, name, drop):
    """Case `name` of acquire_ref.CASES at tau = 0 with `drop` samples deleted
    at sample (ns // 2) n. Returns (x, truth, cut, phase2): two segments split
    at window `cut` (a multiple of R at or before the slip), the second's
    expected phase ((n - drop) % n) / hop, the first's being 0."""
    freqs, n, hop, ns = acquire_ref.CASES[name][:4]
    R = n // hop
    x, truth = acquire_ref.case_stream(O, name, 0)
    at = (ns // 2) * n
    x = np.ascontiguousarray(np.concatenate([x[:at], x[at + drop:]]))
    cut = (at // hop) // R * R
    return x, truth, cut, ((n - drop) % n) // hop
