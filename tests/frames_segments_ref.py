"""Numpy restatement of the segmented frame scan (include/demod.h, "segmented
frame scan"): the reference of tests/test_frames_segments_cpu.py and
tests/test_gpu_frames_segments.py.

Segment s of a batch sym[Wb], P[Wb][K] is windows first[s] .. first[s] +
count[s] - 1 and is scanned as a batch of its own by frames_ref.frames on the
slice (window indices relative to first'), after the rules of
acquire_segments_ref, restated for this call's tile words:

  the clamp        first' = min(first, Wb), count' = min(count, Wb - first');
  the short rule   count' < R: phases R, phase 0, per_phase 0, metric all 0,
                   n_hits = n_written = 0, tail_window -1, tail_errors 0, no rows;
  the tile budget  a segment of count' >= R windows has ceil(count' / tile)
                   tiles; segment s is scanned when the tiles of segments 0 .. s
                   together are <= budget, else it is reported as a short one.
                   A tile's words are 16 R + 4 R + 4 bytes, each array padded
                   to 8 (tiles_bytes); a call's budget is the largest B whose
                   words its work_bytes hold beyond the header (budget_of).
"""
import numpy as np

import acquire_segments_ref as SR
import frames_ref as F

TILE = SR.TILE


def header_bytes(S):
    """acquire_seg_header_bytes: first' (8 bytes) and count', first tile, tiles
    (4 bytes each) per segment, the call's total (4 bytes), padded to 8."""
    return (20 * int(S) + 4 + 7) // 8 * 8


def tiles_bytes(B, R):
    """part and tail [B][R] (8 bytes each), count [B][R] and offs [B] (4 bytes
    each), every array padded to 8."""
    B, R = int(B), int(R)
    return 16 * B * R + (4 * B * R + 7) // 8 * 8 + (4 * B + 7) // 8 * 8


def workspace_size(R, max_segments, max_windows, tile=TILE):
    """The documented formula of demod_frames_segments_workspace_size."""
    return header_bytes(max_segments) + tiles_bytes(SR.budget_for(max_segments, max_windows, tile), R)


def budget_of(work_bytes, R, n_segments):
    """The largest B with header_bytes(n_segments) + tiles_bytes(B, R) <= work_bytes."""
    avail = int(work_bytes) - header_bytes(n_segments)
    B = max(avail, 0) // (20 * R + 4)
    while B > 0 and tiles_bytes(B, R) > avail:
        B -= 1
    return B


def short_result(R):
    return dict(metric=np.zeros(R, np.float64), phases=R, phase=0, per_phase=0, n_hits=0, n_written=0,
                tail_window=-1, tail_errors=0, reserved=0)


def empty_rows(N, K):
    B = (N * F.bits_per_symbol(K) + 7) // 8
    return np.zeros(0, F.HIT_DTYPE), np.zeros((0, N), np.uint8), np.zeros((0, B), np.uint8)


def frames_segments(sym, P, R, first, count, sync, max_errors, N, max_frames=None, budget=None, tile=TILE):
    """[(hits, payload, packed, result dict)] per segment, as frames_ref.frames
    gives them on the slice."""
    sym = np.asarray(sym, np.uint8).reshape(-1)
    P = np.asarray(P)
    Wb, K = sym.size, P.shape[1]
    assert len(first) == len(count)
    res, used = [], 0
    for f, c in zip(first, count):
        f, c = SR.clamp(f, c, Wb)
        tiles = -(-c // tile) if c >= R else 0
        used += tiles
        if tiles == 0 or (budget is not None and used > budget):
            res.append(empty_rows(N, K) + (short_result(R),))
        else:
            res.append(F.frames(sym[f:f + c], P[f:f + c], R, sync, max_errors, N, max_frames))
    return res


# ---- the slip scenario: n / 2 samples deleted two symbols before the third frame

def slip_stream(freqs, n=1024, hop=256, frame=2):
    """frames_ref.frame_stream at tau = 0 with n / 2 samples deleted two symbols
    before frame `frame`'s word. Returns (x, word, payloads, cut, windows): two
    segments split at window `cut` (a multiple of R at or before the slip), and
    each planted word's first window relative to its own segment, the frames
    after the slip on phase (n / 2) / hop."""
    R = n // hop
    x, word, payloads, windows = F.frame_stream(freqs, 0, n=n, hop=hop)
    at = (int(windows[frame]) // R - 2) * n            # a symbol boundary, in samples
    drop = n // 2
    x = np.ascontiguousarray(np.concatenate([x[:at], x[at + drop:]]))
    cut = (at // hop) // R * R
    moved = windows - drop // hop                      # where the later words now start
    rel = [int(w) if i < frame else int(moved[i]) - cut for i, w in enumerate(windows)]
    return x, word, payloads, cut, rel
