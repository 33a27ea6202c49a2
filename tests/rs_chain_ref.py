"""The host chain of a frame with the Reed-Solomon outer code, for the GPU
tests (tests/test_gpu_rs.py): the scan of (sym, P) by tests/frames_ref.py, the
soft values by tests/frames_fec_ref.py, then the library's host functions
demod_fec_frame_decode (the Viterbi part), demod_rs_frame_decode (the outer
code) and the check of tests/frames_check_ref.py with the length bound that
follows n' and the span of tests/fec_modes_ref.py. Also the symbol
streams these tests send: frames in any of the 20 modes from
demod_tx_frame_symbols, with wrong symbols planted.
"""
import numpy as np

import fec_modes_ref as Z
import frames_check_ref as C
import frames_fec_ref as X
import frames_ref as F
import rs_ref as R


def row_width(A, N, bits, h, fec):
    """W: B of the packed rows, or Bd of the decoded rows in a coded mode."""
    return A.fec_row_bytes(N, bits, h, fec & 0xFF) if fec & 0xFF else (N * bits + 7) // 8


def max_len(A, N, bits, h, kind, fec):
    return R.max_len(row_width(A, N, bits, h, fec), h, C.CRC_BYTES[kind], R.mode_parity(fec))


def rows_of(A, sym, P, hits, L, Rn, N, h, kind, fec, poison=0):
    """The rows the outer code's stage reads: the scan's packed rows, or the
    Viterbi decoder's rows (bytes it does not write are `poison`)."""
    W, K = P.shape
    bits = F.bits_per_symbol(K)
    width = row_width(A, N, bits, h, fec)
    rows = np.full((len(hits), width), poison, np.uint8)
    if fec & 0xFF:
        soft = X.soft_bits(P)
        for i, w in enumerate(hits["window"]):
            written, _ = A.fec_frame_decode(X.row_soft(soft, W, 0, int(w), L, Rn, N), h, kind, fec)
            rows[i, :len(written)] = np.frombuffer(written, np.uint8)
    else:
        pay = sym[hits["window"].astype(np.int64)[:, None] + Rn * (L + np.arange(N))[None, :]].reshape(len(hits), N)
        packed = F.pack(pay, bits)
        rows[:] = np.asarray(packed, np.uint8).reshape(len(hits), width)
    return rows


def outer(A, rows, h, kind, fec):
    """demod_rs_frame_decode over every row: (rows, records FRAME_RS_DTYPE)."""
    out = rows.copy()
    rec = np.zeros(len(rows), A.FRAME_RS_DTYPE)
    for i in range(len(rows)):
        got, r, _ = A.rs_frame_decode(rows[i], h, kind, fec)
        out[i] = got
        rec[i] = tuple(r[f] for f in A.FRAME_RS_DTYPE.names)
    return out, rec


def chain(A, sym, P, Rn, word, max_errors, N, h, kind, fec):
    """Scan, decode, outer decode, check on one batch: (hits, rows before the
    outer code, rows after, records, check_group's four, the scan's result)."""
    hits, _, _, res = F.frames(sym, P, Rn, word, max_errors, N)
    bits = F.bits_per_symbol(P.shape[1])
    before = rows_of(A, np.asarray(sym, np.uint8), P, hits, len(word), Rn, N, h, kind, fec)
    after, rec = outer(A, before, h, kind, fec)
    chk = C.check_group(hits["window"], after, len(word), Rn, Z.span_of(bits, h, kind, fec),
                        max_len(A, N, bits, h, kind, fec), h, kind)
    return hits, before, after, rec, chk, res


def stream_symbols(A, K, fec, h, kind, datas, N, word, plant, rng, lead=9, gaps=None):
    """The frames `datas` in the mode (demod_tx_frame_symbols) among random
    symbols, each padded to N payload symbols; plant(f, Sp, rng) lists the
    payload symbols of frame f that go on a wrong tone. Returns (symbols, the
    words' symbol indices)."""
    x = A.make_tx_cfg(word, h, kind, fec, max(len(d) for d in datas), 0, (0,), 8000, 0, 0, 1 << 20, 1, 8)
    seq, at = [rng.integers(0, K, lead).astype(np.uint8)], []
    for f, data in enumerate(datas):
        at.append(sum(len(s) for s in seq))
        frame = A.tx_frame_symbols(x, K, data)
        Sp = len(frame) - len(word)
        row = np.concatenate([frame[len(word):], rng.integers(0, K, N - Sp).astype(np.uint8)])
        for j in plant(f, Sp, rng):
            row[j] = (row[j] + 1 + int(rng.integers(0, K - 1))) % K
        gap = (8 + 3 * f) if gaps is None else gaps[f]
        seq += [np.asarray(word, np.uint8), row, rng.integers(0, K, gap).astype(np.uint8)]
    seq.append(rng.integers(0, K, 4).astype(np.uint8))
    return np.concatenate(seq), at


def pcm_of(freqs, truth, seed, n=1024, sigma=400.0, amplitude=8000.0):
    """The symbols as FSK with a random phase per symbol plus Gaussian noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    ph = rng.uniform(0, 2 * np.pi, truth.size)
    w = 2 * np.pi * np.asarray(freqs, np.float64)[truth] / 48000.0
    x = np.empty((truth.size, n), np.int16)
    for a in range(0, truth.size, 512):
        v = amplitude * np.sin(w[a:a + 512, None] * t[None, :] + ph[a:a + 512, None]) + \
            rng.normal(0.0, sigma, (len(w[a:a + 512]), n))
        x[a:a + 512] = np.clip(np.round(v), -32768, 32767)
    return np.ascontiguousarray(x.reshape(-1))
