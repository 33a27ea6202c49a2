"""Numpy restatement of the acquisition's definitions (include/demod.h,
"acquisition"): the reference of tests/test_acquire_cpu.py and
tests/test_gpu_acquire.py.

Inputs are a detector batch's outputs, sym[W] (uint8) and P[W][K], window w at
sample w hop, R = n / hop phases, J = floor(W / R):

  M[r]         = sum_{j < J} (double) P[jR + r][sym[jR + r]]; a byte >= K adds
                 nothing; the tail w >= J R is left out. Summed with math.fsum,
                 i.e. correctly rounded: the exact sum to half an ulp, so a
                 sum of the same non-negative doubles in ANY order is within
                 (J - 1) 2^-53 (1 + o(1)) M of it, inside the tests' J 2^-52 M.
  phase        = argmax M, ties to the lowest.
  errors(w)    = #{i : sym[w + iR] != sync[i]} for w + (len - 1) R < W.
  sync_window  = the lowest w = phase (mod R) with errors(w) <= max_errors,
                 else -1; sync_errors = errors(sync_window) (0 if none).
  first_window = sync_window + len R; phase if len == 0; W if not found.
  n_out        = #{j >= 0 : first_window + jR < W}; out = sym[first_window::R].
"""
import math

import numpy as np

# demod_acquire_result_t, restated from the header: the one layout the tests read results with
RESULT_DTYPE = np.dtype([("metric", "<f8", 64), ("phases", "<u4"), ("phase", "<u4"),
                         ("per_phase", "<u8"), ("sync_window", "<i8"), ("sync_errors", "<u4"),
                         ("reserved", "<u4"), ("first_window", "<u8"), ("n_out", "<u8"),
                         ("n_written", "<u8")])
assert RESULT_DTYPE.itemsize == 568


def phase_metric(sym, P, R):
    sym = np.asarray(sym, np.uint8).reshape(-1)
    P = np.asarray(P)
    W, K = P.shape
    assert sym.size == W and W >= R >= 1
    J = W // R
    ok = sym[:J * R] < K
    idx = np.where(ok, sym[:J * R], 0).astype(np.int64)
    v = np.where(ok, P[np.arange(J * R), idx].astype(np.float64), 0.0).reshape(J, R)
    return np.array([math.fsum(v[:, r]) for r in range(R)], np.float64), J


def sync_errors(sym, R, sync, w):
    """errors(w), or None where the word would run past the batch."""
    L = len(sync)
    if w + (L - 1) * R >= len(sym):
        return None
    return int(np.count_nonzero(np.asarray(sym)[w:w + L * R:R] != np.asarray(sync, np.uint8)))


def acquire(sym, P, R, sync=(), max_errors=0, cap=None, metric=None):
    """Returns (out, result dict) as Demodulator.acquire does; out is the whole
    stream sym[first_window::R] cut to cap (None: uncut). metric: (M, J) of an
    earlier phase_metric(sym, P, R) call, for callers that change only symbols
    the metric does not depend on."""
    sym = np.asarray(sym, np.uint8).reshape(-1)
    W = sym.size
    sync = np.asarray(sync, np.uint8).reshape(-1)
    L = sync.size
    M, J = phase_metric(sym, P, R) if metric is None else metric
    phase = int(np.argmax(M))          # the first maximum: ties to the lowest
    sync_window, errs = -1, 0
    if L:
        assert max_errors < L
        # errors of every legal start on the phase, vectorised
        last = W - 1 - (L - 1) * R
        starts = np.arange(phase, last + 1, R, dtype=np.int64)
        if starts.size:
            e = (sym[starts[:, None] + R * np.arange(L)[None, :]] != sync[None, :]).sum(axis=1)
            hit = np.flatnonzero(e <= max_errors)
            if hit.size:
                sync_window, errs = int(starts[hit[0]]), int(e[hit[0]])
        first = sync_window + L * R if sync_window >= 0 else W
    else:
        first = phase
    out = sym[first::R] if first < W else sym[:0]
    n_out = int(out.size)
    n_written = n_out if cap is None else min(n_out, int(cap))
    res = dict(metric=M, phases=R, phase=phase, per_phase=J, sync_window=sync_window,
               sync_errors=errs, reserved=0, first_window=first, n_out=n_out, n_written=n_written)
    return out[:n_written].copy(), res


def margin(M):
    """Best-vs-second phase margin as a fraction of the best (1.0 for R = 1)."""
    if len(M) < 2:
        return 1.0
    s = np.sort(np.asarray(M, np.float64))
    return float((s[-1] - s[-2]) / s[-1])


# ---- the end-to-end cases (tests/test_acquire_cpu.py, tests/test_gpu_acquire.py)
# name: (freqs, n, hop, symbols generated, noise sigma, table margin with tau on
# a multiple of hop, table margin at tau = 2 hop + hop / 4)
CASES = {
    "A": ((1500.0, 3000.0), 1024, 256, 300, 400, 0.43, 0.24),
    "B": ((1500.0, 3000.0), 1024, 64, 42, 2000, 0.13, 0.066),
    "C": (tuple(1500.0 + 375.0 * i for i in range(4)), 256, 64, 300, 2000, 0.42, 0.25),
    "D": (tuple(375.0 * (4 + i) for i in range(8)), 1024, 256, 120, 2000, 0.43, 0.25),
}
CASE_SEED = 0x2C5DA044


def case_taus(n, hop):
    """[(tau, phase expected)]: tau on multiples of hop (0, hop, (R - 1) hop,
    3 hop where R > 3), then 2 hop + hop / 4 (the nearer phase, 2)."""
    R = n // hop
    on = sorted({0, hop, (R - 1) * hop} | ({3 * hop} if R > 3 else set()))
    return [(t, t // hop) for t in on] + [(2 * hop + hop // 4, 2)]


def case_stream(O, name, tau):
    """The case's FSK stream cut so that a symbol boundary lies at sample tau
    (0 <= tau < n). Returns (x int16, truth): truth[i] is the symbol that
    starts at sample tau + i n."""
    freqs, n, hop, ns, sigma, _, _ = CASES[name]
    pcm, truth = O.synth_fsk(freqs, n, ns, CASE_SEED, sigma=sigma)
    x = pcm.reshape(-1)
    if tau:
        return np.ascontiguousarray(x[n - tau:]), truth[1:]
    return np.ascontiguousarray(x), truth


# ---- test-made inputs (tests/test_gpu_acquire.py, tests/test_gpu_acquire_segments.py) -------

def make_inputs(W, K, Rn, seed, boost=None, flat=False):
    """sym random < K; P random positive fp32 over 1e0 .. 1e14, phase `boost`'s
    powers scaled by 1.5. flat: every tone of a window the same power, so the
    metric does not depend on the symbols (the sync tests plant symbols)."""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, K, W).astype(np.uint8)
    P = (10.0 ** rng.uniform(0.0, 14.0, (W, 1 if flat else K))).astype(np.float32)
    if flat:
        P = np.repeat(P, K, axis=1)
    if boost is not None:
        P[boost::Rn] *= np.float32(1.5)
    return sym, np.ascontiguousarray(P)


def plant(sym, Rn, w0, word, n_bad, K, rng):
    """word on sym[w0 :: Rn] with exactly n_bad mismatching positions, each
    another symbol < K (K >= 2), so that with tone-independent powers the
    metric stays what it was."""
    assert K >= 2 or n_bad == 0
    s = sym.copy()
    L = len(word)
    s[w0:w0 + L * Rn:Rn] = word
    for pos in rng.choice(L, n_bad, replace=False):
        s[w0 + pos * Rn] = (int(word[pos]) + 1 + int(rng.integers(0, K - 1))) % K
    return s
