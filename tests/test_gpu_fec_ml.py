"""The device's Viterbi decoder (frames_fec.hip) against the independent
maximum-likelihood reference of tests/fec_ml_ref.py.

tests/test_gpu_frames_fec.py compares the device with tests/frames_fec_ref.py
on loud tones with four flipped bits. Here the powers are weak, contradictory,
erased and tied, and after the same whole comparison (rows and decode records
over the poison) the device's own bytes are held to fec_ml_ref.check_decodes:
the path it wrote attains the greatest correlation of any code path.

K = 2: the powers [127 + q, 127 - q] give the soft value q exactly (127 * 2 q
/ 254 in double), so the families of tests/test_fec_ml_cpu.py reach the device
value for value, one soft value a window. K = 4, 8, 16: exponential(1) powers
with the sent tone raised by 2, 3 or 5; the soft values are what
demod_soft_bits makes of them.
"""
import numpy as np
import pytest

import fec_ml_ref as ML
import fec_modes_ref as Z
import frames_check_ref as C
import frames_fec_ref as X
import frames_ref as F
import test_fec_ml_cpu as M
from test_gpu_frames_fec import (L0, Run, frame_symbols, handle, info_symbols, lay_rows, min_symbols,  # noqa: F401
                                 one_group, reference, same, torch)

pytestmark = pytest.mark.gpu


def lay_soft(q, Rn, rng):
    """K = 2: the rows' soft values q [n][C] as powers, laid by lay_rows."""
    P, starts = lay_rows([(row < 0).astype(np.uint8) for row in q], 2, Rn, rng)
    for row, s in zip(q, starts):
        w = int(s) + (L0 + np.arange(q.shape[1])) * Rn
        P[w, 0], P[w, 1] = 127.0 + row, 127.0 - row
    return P, starts


def lay_tones(rows_sym, K, Rn, rng, boost):
    """The rows' symbols laid by lay_rows, the powers redrawn: exponential(1),
    the sent tone (everywhere, the random symbols between the rows too) raised
    by `boost`."""
    P, starts = lay_rows(rows_sym, K, Rn, rng)
    sym = np.argmax(P, axis=1)
    P = rng.exponential(1.0, P.shape).astype(np.float32)
    P[np.arange(len(P)), sym] += np.float32(boost)
    return P, starts


def run_and_check(A, torch, d, P, starts, Rn, N, h, kind, what, decoder=None):
    """One group of len(starts) rows through the device: rows and decode
    records whole against reference(), then check_decodes on the device's own
    bytes. Returns (q [n][C], the OK rows, steps)."""
    n, c = len(starts), C.CRC_BYTES[kind]
    hits = one_group(starts, n + 2)
    want = reference(P, len(P), None, hits, [n], L0, Rn, N, h, kind, decoder=decoder)
    got = Run(A, torch, P, hits, [n])(d, L0, N, h, kind)
    same(got, want[:2], what)
    soft = X.soft_bits(P)
    q = np.array([X.row_soft(soft, len(P), 0, s, L0, Rn, N) for s in starts])
    dec = np.ascontiguousarray(got[1][0, :n]).view(ML.DECODE_DTYPE).reshape(-1)
    Bd = got[0].shape[2]
    count = np.where(dec["status"] == ML.OK, np.minimum(h + dec["length"].astype(np.int64) + c, Bd), h)
    written = [got[0][0, i, :int(count[i])].tobytes() for i in range(n)]
    ok, steps = ML.check_decodes(q, h, c, written, dec, ("device",) + tuple(what))
    return q, ok, steps


@pytest.mark.parametrize("Rn", [1, 4])
@pytest.mark.parametrize("case", M.CASES)
def test_two_tones_value_for_value(A, torch, handle, case, Rn):
    """The cases of tests/test_fec_ml_cpu.py on the device, each batch one
    group: 7 rows of 2070 steps for most, 65 for the codewords from the other
    64 start states, 38 rows each for the h 2 row and the four minimal rows
    (two of them with an odd soft count)."""
    d = handle(Rn, 2)
    batches = M.case_batches(case)
    oks, steps = [], []
    for b, (h, kind, q) in enumerate(batches):
        rng = np.random.default_rng(100 * M.CASES.index(case) + 10 * b + Rn)
        P, starts = lay_soft(q, Rn, rng)
        got_q, ok, st = run_and_check(A, torch, d, P, starts, Rn, q.shape[1], h, kind, (case, b, Rn))
        assert np.array_equal(got_q, q), "the powers do not give the soft values they were made from"
        oks.append(ok)
        steps.append(st)
    if case == "other-starts":
        assert len(batches[0][2]) == 65
    M.fixture_holds(case, batches, oks, steps)


def tone_rows(rng, n, N, bits, h, kind):
    """n coded frames, their lengths spread over 0 .. max_len, as row symbols."""
    max_len = X.row_shape(N, bits, h, kind)[2]
    lens = (M.spread(max_len, 12) * n)[:n]
    return [frame_symbols(rng, length, N, bits, h, kind, flips=0)[0] for length in lens]


@pytest.mark.parametrize("boost", [2, 3, 5])
@pytest.mark.parametrize("Rn", [1, 4])
@pytest.mark.parametrize("K", [4, 8, 16])
def test_noisy_tones(A, torch, handle, K, Rn, boost):
    """24 frames in rows of 2070 steps, 8 in the h 2 row of max_len 24 and 8
    in the minimal row, their tones raised by `boost` over exponential(1)
    noise (at 8 tones a boost of 2 leaves a third of the hard symbols wrong).
    At boost 2 a third of the soft values or more (at 4 tones a quarter) are at
    most 32 in size: the fixture is not the +-127 regime."""
    d = handle(Rn, K)
    bits = F.bits_per_symbol(K)
    rng = np.random.default_rng(1000 * K + 10 * Rn + boost)
    shapes = [(M.LONG[0], M.LONG[1], Z.symbols_for(M.LONG[2], bits, *M.LONG[:2], X.CONV_K7), 24),
              (M.H2[0], M.H2[1], Z.symbols_for(M.H2[2], bits, *M.H2[:2], X.CONV_K7), 8),
              (1, C.CRC16, min_symbols(bits, 1), 8)]
    oks, steps, small = [], [], []
    for h, kind, N, n in shapes:
        P, starts = lay_tones(tone_rows(rng, n, N, bits, h, kind), K, Rn, rng, boost)
        q, ok, st = run_and_check(A, torch, d, P, starts, Rn, N, h, kind, (K, Rn, boost, N))
        some = rng.integers(0, len(P), 200)
        assert np.array_equal(np.array([A.soft_bits(P[w]) for w in some]), X.soft_bits(P[some]))
        oks.append(ok)
        steps.append(st)
        small.append(np.abs(q.astype(np.int32)) <= 32)
    assert oks[0].all()
    ok, st = np.concatenate(oks), np.concatenate(steps)
    assert 2 * int(ok.sum()) >= ok.size and len(set(st[ok].tolist())) >= 4, (int(ok.sum()), sorted(set(st[ok].tolist())))
    if boost == 2:
        # of these powers alone, whatever decodes them: 47 % at 8 tones and 62 % at 16, but 31 % at 4, where
        # each maximum is over two tones only; there a quarter is asked for
        part = 3 if K >= 8 else 4
        assert part * int(sum(s.sum() for s in small)) >= sum(s.size for s in small)


def test_longest_rows(A, torch, handle):
    """Two rows of 32822 steps at 16 tones (max_len 4096, h 2, CRC-32), the
    sent tone 1 and the others 0 where a soft value is to be +-127: the negated
    codeword of tests/test_fec_ml_cpu.py::longest_negated, and a row of
    exponential(1) noise behind the first 8 h + 64 steps of a frame of length
    4096, so that its header is valid and all 32822 steps of noise are decoded.
    The whole comparison is against the host decoder, as
    tests/test_gpu_frames_fec.py::test_longest_row's is."""
    K, Rn, bits = 16, 1, 4
    rng = np.random.default_rng(32822)
    q5, h, kind = M.longest_negated(rng)
    N = Z.symbols_for(4096, bits, h, kind, X.CONV_K7)
    assert N * bits == q5.size and X.row_shape(N, bits, h, kind)[::2] == (32822, 4096)
    weights = np.array([8, 4, 2, 1])
    sym5 = ((q5 < 0).reshape(N, bits) * weights).sum(axis=1).astype(np.uint8)
    t0 = 8 * h + ML.DEPTH
    head = info_symbols((4096).to_bytes(h, "big") + rng.integers(0, 256, 16).astype(np.uint8).tobytes(), t0, N, bits,
                        rng, 0)
    P, starts = lay_rows([sym5, head], K, Rn, rng)
    noise = rng.exponential(1.0, P.shape).astype(np.float32)
    w5 = int(starts[0]) + (L0 + np.arange(N)) * Rn
    w1 = int(starts[1]) + (L0 + np.arange(2 * t0 // bits)) * Rn
    keep = np.zeros(len(P), bool)
    keep[w5], keep[w1] = True, True
    P = np.where(keep[:, None], (P >= 1000).astype(np.float32), noise)
    q, ok, st = run_and_check(A, torch, handle(Rn, K), P, starts, Rn, N, h, kind, ("longest",),
                              decoder=A.coded_frame_decode)
    assert np.array_equal(q[0], q5) and np.abs(q[1, :2 * t0]).min() == 127
    assert ok.all() and st.tolist() == [M.LONGEST_NEGATED_STEPS, 32822]
    assert (np.abs(q[1, 2 * t0:].astype(np.int32)) <= 32).mean() > 0.1
