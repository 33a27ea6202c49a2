"""An independent maximum-likelihood reference for the coded frame's decoder
(include/demod.h "coded frames"): the reference of tests/test_fec_ml_cpu.py
and tests/test_gpu_fec_ml.py.

Everything here follows from the encoder's definition alone: reg_-1 = 0, reg_t
= ((reg_t-1 << 1) | u_t) & 0x7F, v_2t = parity(reg_t & 0171), v_2t+1 =
parity(reg_t & 0133). The transition table is made by running that update for
every (register, input); the predecessors of a state are read back out of the
table. Nothing is taken from tests/frames_fec_ref.py or from the decoders: no
p0 / p1 rule, no "second branch is minus the first", no metric floor.

best(q, T, fixed, end) is the greatest correlation sum_m q[m] (1 - 2 v[m]) over
the code paths of T steps from state 0, in int64, with states that no path
reaches held at UNREACHABLE (re-pinned every step, so that no sum of soft
values lifts one into the race). A Viterbi decoder is right exactly when the
path it returns attains that maximum: check_decodes states it as "the optimum
with the decoded bits forced equals the free optimum", which any optimal path
passes, so ties need no exclusions.
"""
import numpy as np

G0, G1 = 0o171, 0o133                  # include/demod.h
DEPTH = 64                             # DEMOD_FEC_DEPTH
OK, BAD_LENGTH = 0, 1                  # DEMOD_DECODE_OK, DEMOD_DECODE_BAD_LENGTH
DECODE_DTYPE = np.dtype([("length", "<u4"), ("metric", "<i4"), ("status", "<u4"), ("steps", "<u4")])
UNREACHABLE = -(1 << 62)


def parity(v):
    return bin(v).count("1") & 1


def register_step(reg, u):
    """One step of the header's encoder: (reg_t, v_2t, v_2t+1)."""
    reg = ((reg << 1) | u) & 0x7F
    return reg, parity(reg & G0), parity(reg & G1)


def _table():
    nxt = np.zeros((64, 2), np.int64)
    signs = np.zeros((64, 2, 2), np.int64)
    for s in range(64):
        for u in (0, 1):
            # the register's bit 6 leaves with the shift: the state is reg & 63
            both = {register_step(s | top, u) for top in (0, 64)}
            assert len(both) == 1
            reg, v0, v1 = both.pop()
            nxt[s, u] = reg & 63
            signs[s, u] = (1 - 2 * v0, 1 - 2 * v1)
    return nxt, signs


NEXT, SIGNS = _table()                 # next[state][u], signs[state][u][2] = 1 - 2 v
_FLAT_NEXT = NEXT.reshape(-1)          # branch s * 2 + u
_PRED = np.array([np.flatnonzero(_FLAT_NEXT == d) for d in range(64)])      # [64][2] branches into d
assert _PRED.shape == (64, 2)
_SRC = np.arange(128) // 2
_U = np.arange(128) % 2
_S0, _S1 = SIGNS[:, :, 0].reshape(-1), SIGNS[:, :, 1].reshape(-1)


def walk(u):
    """The 2 len(u) coded bits of the inputs u from state 0, through the table."""
    out = np.zeros(2 * len(u), np.uint8)
    s = 0
    for t, b in enumerate(u):
        out[2 * t], out[2 * t + 1] = (1 - SIGNS[s, int(b)]) // 2
        s = int(NEXT[s, int(b)])
    return out


def first_event_spectrum(max_weight):
    """{weight: (paths, information bits)} of the paths that leave state 0 and
    first return to it, by a walk of the table."""
    spectrum = {}
    w0 = int((SIGNS[0, 1] < 0).sum())
    front = {(int(NEXT[0, 1]), w0): (1, 1)}             # (state, weight) -> (paths, their information bits)
    for _ in range(64 * (max_weight + 1)):              # no weightless loop away from state 0: the front dies out
        if not front:
            return spectrum
        new = {}
        for (s, w), (paths, ones) in front.items():
            for u in (0, 1):
                w2 = w + int((SIGNS[s, u] < 0).sum())
                if w2 > max_weight:
                    continue
                d, add = int(NEXT[s, u]), (paths, ones + u * paths)
                if d == 0:
                    old = spectrum.get(w2, (0, 0))
                    spectrum[w2] = (old[0] + add[0], old[1] + add[1])
                else:
                    old = new.get((d, w2), (0, 0))
                    new[d, w2] = (old[0] + add[0], old[1] + add[1])
        front = new
    raise AssertionError("a weightless loop away from state 0")


def best(q, T, fixed=(), end=None):
    """max over u[0 .. T) of sum_m q[m] (1 - 2 v[m]), m < 2 T, from state 0.

    q [2 T or more] or [n][..]: one numpy step per trellis step for all rows.
    T: the steps, one number or one per row. fixed: u[t] = fixed[t] for t <
    len(fixed), one sequence for all rows or [n][F] with -1 where a row's bit is
    free. end: None, or the state the path must end in. Returns int64 (one
    number for a 1-d q), UNREACHABLE where no path satisfies the constraints."""
    q = np.asarray(q)
    single = q.ndim == 1
    q = np.atleast_2d(q).astype(np.int64)
    n = q.shape[0]
    T = np.broadcast_to(np.asarray(T, np.int64), (n,))
    assert (T >= 0).all() and 2 * int(T.max()) <= q.shape[1]
    fixed = np.asarray(fixed, np.int64)
    if fixed.ndim == 1:
        fixed = np.broadcast_to(fixed, (n, fixed.size))
    assert fixed.shape[0] == n and fixed.min(initial=0) >= -1 and fixed.max(initial=0) <= 1

    def take(M):
        return M.max(axis=1) if end is None else M[:, end].copy()

    M = np.full((n, 64), UNREACHABLE, np.int64)
    M[:, 0] = 0
    out = np.where(T == 0, take(M), UNREACHABLE)
    stops = set(T.tolist())
    for t in range(int(T.max())):
        cand = M[:, _SRC] + q[:, 2 * t, None] * _S0 + q[:, 2 * t + 1, None] * _S1      # [n][128]
        if t < fixed.shape[1]:
            f = fixed[:, t, None]
            cand[(f >= 0) & (_U[None, :] != f)] = UNREACHABLE
        M = cand[:, _PRED].max(axis=2)
        M[M < UNREACHABLE // 2] = UNREACHABLE
        if t + 1 in stops:
            out = np.where(T == t + 1, take(M), out)
    return out[0] if single else out


def enumerate_best(q, T, fixed=(), end=None):
    """best() for one row by trying all 2^T inputs through the shift register."""
    top = None
    for word in range(1 << T):
        u = [(word >> (T - 1 - t)) & 1 for t in range(T)]
        if any(u[t] != f for t, f in enumerate(fixed)):
            continue
        reg, total = 0, 0
        for t in range(T):
            reg, v0, v1 = register_step(reg, u[t])
            total += int(q[2 * t]) * (1 - 2 * v0) + int(q[2 * t + 1]) * (1 - 2 * v1)
        if end is not None and reg & 63 != end:
            continue
        top = total if top is None or total > top else top
    return UNREACHABLE if top is None else top


def records(dicts):
    """A list of decode records as dicts -> DECODE_DTYPE [n]."""
    return np.array([tuple(d[f] for f in DECODE_DTYPE.names) for d in dicts], DECODE_DTYPE)


def _bits(data, width):
    """bytes -> `width` entries, the bits MSB first, -1 behind them."""
    b = np.unpackbits(np.frombuffer(bytes(data), np.uint8)).astype(np.int64)
    return np.concatenate([b, np.full(width - b.size, -1, np.int64)])


def check_decodes(q, h, crc_bytes, written, dec, who):
    """The decoder's contract, as far as it follows from the code: q int8
    [n][C], written[r] the bytes the decoder `who` wrote to row r, dec
    DECODE_DTYPE [n].

    header  best(q, t0, fixed = the bits of the decoded length) == best(q, t0),
            t0 = 8 h + 64; status is OK exactly when length <= max_len.
    OK      steps == T = max(8 n + 6, t0), n = h + length + c bytes written (the
            trace over all T steps may revise the look-ahead's header bits);
            best(q, T, fixed = the 8 n written bits, end = 0) == best(q, T,
            end = 0) == metric.
    BAD     metric == 0, steps == 0, the h header bytes alone written.
    Returns (the OK rows as a mask, steps)."""
    q = np.atleast_2d(np.asarray(q))
    n, C = q.shape
    St, t0 = C // 2, 8 * h + DEPTH
    max_len = (St - 6) // 8 - h - crc_bytes
    assert len(written) == n == len(dec) and St >= t0 and max_len >= 0
    length, status = dec["length"].astype(np.int64), dec["status"]
    heads = [int(v).to_bytes(h, "big") for v in length]
    forced = best(q, t0, fixed=np.array([_bits(b, 8 * h) for b in heads]))
    free = best(q, t0)
    bad = np.flatnonzero(forced != free)
    assert bad.size == 0, (who, "the header is not on a best path of the first t0 steps", bad[:4].tolist(),
                           length[bad[:4]].tolist(), forced[bad[:4]].tolist(), free[bad[:4]].tolist())
    ok = length <= max_len
    assert np.array_equal(status, np.where(ok, OK, BAD_LENGTH)), (who, "status", status.tolist(), max_len)
    for r in np.flatnonzero(~ok):
        assert (int(dec["metric"][r]), int(dec["steps"][r]), bytes(written[r])) == (0, 0, heads[r]), (who, "BAD row", r)
    rows = np.flatnonzero(ok)
    if rows.size:
        nb = h + length[rows] + crc_bytes
        T = np.maximum(8 * nb + 6, t0)
        assert np.array_equal(dec["steps"][rows], T), (who, "steps", dec["steps"][rows].tolist(), T.tolist())
        for r, k in zip(rows, nb):
            assert len(written[r]) == k, (who, "bytes written", int(r))     # the full trace may revise the header
        bits = np.array([_bits(written[r], 8 * int(nb.max())) for r in rows])
        forced, free = best(q[rows], T, fixed=bits, end=0), best(q[rows], T, end=0)
        metric = dec["metric"][rows].astype(np.int64)
        bad = np.flatnonzero((forced != free) | (free != metric))
        assert bad.size == 0, (who, "the row is not a best path into state 0, or the metric is not its sum",
                               rows[bad[:4]].tolist(), T[bad[:4]].tolist(), forced[bad[:4]].tolist(),
                               free[bad[:4]].tolist(), metric[bad[:4]].tolist())
    return ok, dec["steps"].astype(np.int64)
