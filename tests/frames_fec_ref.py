"""Numpy and Python restatement of the coded frame (include/demod.h "coded
frames"): the reference of tests/test_frames_fec_cpu.py and
tests/test_gpu_frames_fec.py.

The code is the constraint-length-7, rate-1/2 convolutional code 0171/0133
over a checked frame's bytes (tests/frames_check_ref.py): reg_-1 = 0, reg_t =
((reg_t-1 << 1) | u_t) & 0x7F, v_2t = parity(reg_t & 0171), v_2t+1 =
parity(reg_t & 0133), for T(len) = max(8 n + 6, 8 h + 64) steps, u_t = 0 past
the frame's 8 n bits.

Soft value m = j bits + b of a row: from the K powers of symbol j's window, a0
the largest with bit b (MSB first) clear and a1 the largest with it set (each
from the lowest such tone, replaced by a strictly greater value alone), q =
rint(127 (a0 - a1) / (|a0| + |a1|)) in double when the sum is positive and
finite, else 0; a window at or past n_windows gives 0.

The decoder (decode_rows) works on many rows of one shape at once, one numpy
operation per trellis step: int32 metrics from M[0] = 0, M[s] = -2^28; state
s's predecessors p0 = s >> 1 and p1 = p0 | 32; decision 1 only when the p1 sum
is strictly greater; the header from the best state (lowest on ties) at t0 = 8
h + 64; the row from state 0 at T(len).
"""
import numpy as np

import frames_check_ref as C

G0, G1 = 0o171, 0o133
DEPTH = 64
CONV_K7 = 1
OK, BAD_LENGTH = 0, 1
DECODE_DTYPE = np.dtype([("length", "<u4"), ("metric", "<i4"), ("status", "<u4"), ("steps", "<u4")])
_STATES = np.arange(64)
_P0, _P1 = _STATES >> 1, (_STATES >> 1) | 32


def parity(v):
    return bin(v).count("1") & 1


# the branch from p0 into state s has register s (bit 6 clear): its two expected bits as signs
_SG0 = np.array([-1 if parity(s & G0) else 1 for s in range(64)], np.int32)
_SG1 = np.array([-1 if parity(s & G1) else 1 for s in range(64)], np.int32)
assert parity(64 & G0) and parity(64 & G1)          # from p1 both bits are the complements


def steps(length, h, kind):
    """T(len)."""
    return max(8 * (h + length + C.CRC_BYTES[kind]) + 6, 8 * h + DEPTH)


def coded_symbols(length, h, kind, bits):
    """Sc = ceil(2 T / bits)."""
    return (2 * steps(length, h, kind) + bits - 1) // bits


def row_shape(N, bits, h, kind):
    """(St, Bd, max_len) of rows of N symbols, or None where the row is refused."""
    St = N * bits // 2
    if St < 8 * h + DEPTH:
        return None
    Bd = (St - 6) // 8
    max_len = Bd - h - C.CRC_BYTES[kind]
    if max_len < 0 or max_len > 4096:
        return None
    return St, Bd, max_len


def encode_bits(info, T):
    """The 2 T coded bits of the information bytes `info`, one per element."""
    u = np.unpackbits(np.frombuffer(bytes(info), np.uint8))
    out = np.zeros(2 * T, np.uint8)
    reg = 0
    for t in range(T):
        reg = ((reg << 1) | (int(u[t]) if t < u.size else 0)) & 0x7F
        out[2 * t], out[2 * t + 1] = parity(reg & G0), parity(reg & G1)
    return out


def encode(data, h, kind):
    """The coded frame's bytes, or None where the checked frame is refused."""
    frame = C.encode(data, h, kind)
    if frame is None:
        return None
    return np.packbits(encode_bits(frame, steps(len(data), h, kind))).tobytes()


def soft_bits(P):
    """P float32 [W][K], K = 2^bits -> int8 [W][bits]."""
    P = np.asarray(P, np.float32)
    W, K = P.shape
    bits = K.bit_length() - 1
    assert K == 1 << bits and bits >= 1
    out = np.zeros((W, bits), np.int8)
    for b in range(bits):
        mask = 1 << (bits - 1 - b)
        best = []
        for want in (0, mask):
            ks = [k for k in range(K) if (k & mask) == want]
            a = P[:, ks[0]].copy()
            for k in ks[1:]:
                with np.errstate(invalid="ignore"):
                    a = np.where(P[:, k] > a, P[:, k], a)
            best.append(a.astype(np.float64))
        with np.errstate(invalid="ignore", over="ignore"):
            d = best[0] - best[1]
            s = np.abs(best[0]) + np.abs(best[1])
            ok = (s > 0) & np.isfinite(s)
            q = np.rint(127.0 * np.where(ok, d, 0.0) / np.where(ok, s, 1.0))
        out[:, b] = np.where(ok, q, 0.0).astype(np.int8)
    return out


def row_soft(soft, n_windows, base, window, L, R, N):
    """The N bits soft values of the row whose word starts at window base +
    window; soft is soft_bits of the whole batch. Python integers: no wrap."""
    bits = soft.shape[1]
    out = np.zeros((N, bits), np.int8)
    window = int(window)
    if window < n_windows:
        w = int(base) + window + (L + np.arange(N, dtype=np.int64)) * R
        ok = w < n_windows
        out[ok] = soft[w[ok]]
    return out.reshape(-1)


def _forward(q, M, words, t_from, t_to):
    for t in range(t_from, t_to):
        bm = _SG0[None, :] * q[:, 2 * t, None] + _SG1[None, :] * q[:, 2 * t + 1, None]
        a, b = M[:, _P0] + bm, M[:, _P1] - bm
        d = b > a
        M = np.where(d, b, a)
        words[t] = np.packbits(d, axis=1, bitorder="little").view("<u8").reshape(-1)
    return M


def _trace(words, t_end, s, out):
    """t_end [n] steps per row (0: not traced), s [n] start states; u_t into out [n][>= max t_end]."""
    s = s.astype(np.uint64)
    for t in range(int(t_end.max()) - 1, -1, -1):
        act = t < t_end
        out[act, t] = (s[act] & np.uint64(1)).astype(np.uint8)
        d = (words[t] >> s) & np.uint64(1)
        s = np.where(act, (s >> np.uint64(1)) | (d << np.uint64(5)), s)


def decode_rows(soft, h, kind):
    """soft int8 [n][C]. Returns (written: a list of the bytes written to each
    row, from byte 0; decode DECODE_DTYPE [n])."""
    soft = np.asarray(soft, np.int8)
    n, Cc = soft.shape
    St, Bd, max_len = row_shape(1, Cc, h, kind)       # N bits = C
    c, t0 = C.CRC_BYTES[kind], 8 * h + DEPTH
    q = soft.astype(np.int32)
    M = np.full((n, 64), -(1 << 28), np.int32)
    M[:, 0] = 0
    words = np.zeros((St, n), np.uint64)
    M = _forward(q, M, words, 0, t0)
    best = np.argmax(M, axis=1)                       # the first of the greatest: the lowest state
    bits = np.zeros((n, St), np.uint8)
    _trace(words, np.full(n, t0), best, bits)
    length = np.zeros(n, np.int64)
    for t in range(8 * h):
        length = (length << 1) | bits[:, t]
    dec = np.zeros(n, DECODE_DTYPE)
    dec["length"] = length
    good = length <= max_len
    dec["status"] = np.where(good, OK, BAD_LENGTH)
    T = np.where(good, np.maximum(8 * (h + length + c) + 6, t0), 0)
    metric = np.where(T == t0, M[:, 0], 0)
    for t in range(t0, int(T.max()) if good.any() else 0):
        M = _forward(q, M, words, t, t + 1)           # rows with a smaller T: their outputs are taken already
        metric = np.where(T == t + 1, M[:, 0], metric)
    dec["metric"], dec["steps"] = np.where(good, metric, 0), T
    if good.any():
        _trace(words, T, np.zeros(n, np.int64), bits)
    written = []
    for r in range(n):
        if good[r]:
            nb = h + int(length[r]) + c
            written.append(np.packbits(bits[r, :8 * nb]).tobytes())
        else:
            written.append(int(length[r]).to_bytes(h, "big"))
    return written, dec


def decode(soft, h, kind):
    """One row: (the bytes written, its DECODE_DTYPE record)."""
    written, dec = decode_rows(np.asarray(soft, np.int8)[None, :], h, kind)
    return written[0], dec[0]


def hard_soft(bits01, rng=None, tail=0):
    """Coded bits as +-127 soft values (bit 0: +127), `tail` random values behind them."""
    q = np.where(np.asarray(bits01) == 0, 127, -127).astype(np.int8)
    if tail:
        q = np.concatenate([q, rng.integers(-127, 128, tail).astype(np.int8)])
    return q
