"""Numpy restatement of the frame scan's contract (include/demod.h, "frame
scan"): the reference of tests/test_frames_cpu.py and tests/test_gpu_frames.py.

Inputs are a detector batch's outputs, sym[W] (uint8) and P[W][K], R = n / hop
phases; the phase is acquire_ref's (M[r] by math.fsum, argmax, ties to the
lowest). With L = len(sync), N = frame_symbols, bits = bits_per_symbol(K):

  hit          a start w = phase (mod R), w + (L - 1) R < W, with
               errors(w) = #{i : sym[w + iR] != sync[i]} <= max_errors.
  complete     w + (L + N - 1) R < W.
  hits         the complete hits in ascending w (overlapping ones included);
               n_written = min(n_hits, max_frames).
  tail_window  the lowest hit that is not complete, -1 if none; tail_errors
               its errors (0 if none).
  payload[i]   sym[w_i + (L + j) R], j < N (raw bytes).
  packed[i]    payload[i] masked to `bits` bits a symbol, MSB first, padded
               with 0 bits to ceil(N bits / 8) bytes.
"""
import numpy as np

import acquire_ref

HIT_DTYPE = np.dtype([("window", "<u8"), ("errors", "<u4"), ("reserved", "<u4")])
# demod_frames_result_t, restated from the header: the one layout the tests build and read results with
RESULT_DTYPE = np.dtype([("metric", "<f8", 64), ("phases", "<u4"), ("phase", "<u4"), ("per_phase", "<u8"),
                         ("n_hits", "<u8"), ("n_written", "<u8"), ("tail_window", "<i8"),
                         ("tail_errors", "<u4"), ("reserved", "<u4")])
assert RESULT_DTYPE.itemsize == 560


def bits_per_symbol(K):
    """ceil(log2 K), at least 1."""
    return max(1, int(K - 1).bit_length())


def pack(payload, bits):
    """Rows of symbols -> rows of bytes: each symbol's low `bits` bits, MSB
    first, pad bits 0."""
    payload = np.asarray(payload, np.uint8)
    rows, N = payload.shape
    B = (N * bits + 7) // 8
    b = np.unpackbits(payload[:, :, None], axis=2)[:, :, 8 - bits:].reshape(rows, N * bits)
    b = np.concatenate([b, np.zeros((rows, B * 8 - N * bits), np.uint8)], axis=1)
    return np.packbits(b, axis=1).reshape(rows, B)


def frames(sym, P, R, sync, max_errors, N, max_frames=None, metric=None):
    """Returns (hits HIT_DTYPE [n_written], payload uint8 [n_written][N], packed
    uint8 [n_written][B], result dict). metric: (M, J) of an earlier
    acquire_ref.phase_metric(sym, P, R), for callers that change only symbols
    the metric does not depend on."""
    sym = np.asarray(sym, np.uint8).reshape(-1)
    W, K = sym.size, np.asarray(P).shape[1]
    sync = np.asarray(sync, np.uint8).reshape(-1)
    L = sync.size
    assert 1 <= L and max_errors < L and N >= 0
    M, J = acquire_ref.phase_metric(sym, P, R) if metric is None else metric
    phase = int(np.argmax(M))
    starts = np.arange(phase, W - (L - 1) * R, R, dtype=np.int64)       # the word fits
    if starts.size:
        e = (sym[starts[:, None] + R * np.arange(L)[None, :]] != sync[None, :]).sum(axis=1)
    else:
        e = np.zeros(0, np.int64)
    is_hit = e <= max_errors
    complete = starts + (L + N - 1) * R < W
    w_hit, e_hit = starts[is_hit & complete], e[is_hit & complete]
    late = np.flatnonzero(is_hit & ~complete)
    tail_window, tail_errors = (int(starts[late[0]]), int(e[late[0]])) if late.size else (-1, 0)
    n_hits = int(w_hit.size)
    nw = n_hits if max_frames is None else min(n_hits, int(max_frames))
    hits = np.zeros(nw, HIT_DTYPE)
    hits["window"], hits["errors"] = w_hit[:nw], e_hit[:nw]
    payload = sym[w_hit[:nw, None] + R * (L + np.arange(N))[None, :]].reshape(nw, N)
    packed = pack(payload, bits_per_symbol(K))
    res = dict(metric=M, phases=R, phase=phase, per_phase=J, n_hits=n_hits, n_written=nw,
               tail_window=tail_window, tail_errors=tail_errors, reserved=0)
    return hits, payload, packed, res


# ---- the end-to-end stream (tests/test_frames_cpu.py, tests/test_gpu_frames.py)
FRAME_L, FRAME_N, FRAME_COUNT = 24, 64, 5
FRAME_TAUS = (0, 256, 2 * 256 + 256 // 4)      # hop 256: on a window, one hop on, between two
FRAME_SEED = 20241
FSK2 = (1500.0, 3000.0)                         # acquire_ref case A's plan: n 1024, hop 256, sigma 400
FSK8 = tuple(1500.0 + 375.0 * i for i in range(8))   # multiples of 8 bins: the fold detector's plan


def frame_stream(freqs, tau, n=1024, hop=256, sigma=400.0, amplitude=8000.0, seed=FRAME_SEED,
                 fs=48000.0, drop=()):
    """FRAME_COUNT frames of a FRAME_L-symbol word and FRAME_N payload symbols,
    separated (and surrounded) by runs of random symbols, as FSK with a random
    phase per symbol plus Gaussian noise, cut so that a symbol boundary lies at
    sample tau. The frames listed in `drop` carry random symbols in place of
    their word (every other symbol is the same; phases and noise are redrawn).
    Returns (x int16, word, payloads [5][64], windows: each planted word's
    first window on the phase (tau + hop / 2) // hop, dropped frames included)."""
    rng = np.random.default_rng(seed + 7 * len(freqs))
    K, R = len(freqs), n // hop
    word = rng.integers(0, K, FRAME_L).astype(np.uint8)
    payloads = rng.integers(0, K, (FRAME_COUNT, FRAME_N)).astype(np.uint8)
    seq, at = [rng.integers(0, K, 9).astype(np.uint8)], []
    for f in range(FRAME_COUNT):
        at.append(sum(len(s) for s in seq))
        seq += [word, payloads[f], rng.integers(0, K, 5 + 3 * f).astype(np.uint8)]
    truth = np.concatenate(seq)
    t = np.arange(n)
    for f in drop:
        truth[at[f]:at[f] + FRAME_L] = rng.integers(0, K, FRAME_L)
    ph = rng.uniform(0, 2 * np.pi, truth.size)
    w = 2 * np.pi * np.asarray(freqs, np.float64)[truth] / fs
    v = amplitude * np.sin(w[:, None] * t[None, :] + ph[:, None]) + rng.normal(0.0, sigma, (truth.size, n))
    x = np.clip(np.round(v), -32768, 32767).astype(np.int16).reshape(-1)
    phase = (tau + hop // 2) // hop
    if tau:   # symbol i + 1 now starts at sample tau + i n
        x, at = x[n - tau:], [a - 1 for a in at]
    windows = np.array([phase + a * R for a in at], np.int64)
    return np.ascontiguousarray(x), word, payloads, windows
