"""The coded frame's decoders against an independent maximum-likelihood
reference (tests/fec_ml_ref.py), without a GPU.

tests/test_frames_fec_cpu.py holds the host decoder to tests/frames_fec_ref.py
bit for bit; both are one construction. Here the construction itself is held
to what the encoder in include/demod.h defines: the reference against plain
enumeration, the transition table against the encoder and the code's published
weight spectrum, and then both decoders, on noise, weak values, ties, erasures,
low-SNR frames and negated codewords, to "the decoded path attains the greatest
correlation of any code path".
"""
import os
import re

import numpy as np
import pytest

import fec_ml_ref as ML
import fec_modes_ref as Z
import frames_check_ref as C
import frames_fec_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG = (1, C.CRC16, 255)        # h, CRC, max_len: 2070 steps; every 8-bit header is a valid length
H2 = (2, C.CRC32, 24)           # 246 steps


def n_soft(h, kind, max_len):
    """C of the smallest row of one soft value a symbol that holds max_len data bytes."""
    return Z.symbols_for(max_len, 1, h, kind, X.CONV_K7)


# ---- the input families: int8 soft values [n][C] --------------------------------------

def uniform(rng, n, Cs, low=-127):
    return rng.integers(low, 128, (n, Cs)).astype(np.int8)


def weak(rng, n, Cs):
    """rint(N(0, 20)): many zeros and near-ties."""
    return np.rint(rng.normal(0.0, 20.0, (n, Cs))).astype(np.int8)


def codeword(rng, length, h, kind, Cs):
    """The 2 T coded bits (cut at Cs) of a frame of `length` random bytes."""
    info = C.encode(rng.integers(0, 256, length).astype(np.uint8).tobytes(), h, kind)
    return X.encode_bits(info, X.steps(length, h, kind))[:Cs]


def planted(rng, lengths, h, kind, Cs, a, erase=0.0):
    """clip(rint(a (1 - 2 v) + N(0, 30))) over each frame's coded bits, noise
    alone behind them; `erase` of the values set to 0."""
    out = np.zeros((len(lengths), Cs), np.int8)
    for r, length in enumerate(lengths):
        v = codeword(rng, length, h, kind, Cs)
        s = np.zeros(Cs)
        s[:v.size] = a * (1.0 - 2.0 * v)
        q = np.clip(np.rint(s + rng.normal(0.0, 30.0, Cs)), -127, 127)
        q[rng.random(Cs) < erase] = 0
        out[r] = q
    return out


def negated(rng, lengths, h, kind, Cs):
    """-127 (1 - 2 v) of a frame's codeword v, +-127 noise behind it: every
    value speaks against the frame that was sent."""
    out = np.zeros((len(lengths), Cs), np.int8)
    for r, length in enumerate(lengths):
        v = codeword(rng, length, h, kind, Cs)
        out[r] = np.concatenate([-X.hard_soft(v), X.hard_soft(rng.integers(0, 2, Cs - v.size))])
    return out


def other_starts(rng, Cs):
    """Row s, s < 64: the +-127 codeword of random inputs from the register s
    in place of 0. No path from state 0 matches it; a decoder whose other start
    states are not far enough below state 0 follows the path that does. (The
    path of the same inputs from state 0 differs in its first 6 steps alone,
    and the nearest one lies 8 coded bits away for s = 1, 11, 33 and 43: a
    floor within 2 * 127 * 8 of 0 is overtaken, whatever the row's length.)"""
    out = np.zeros((64, Cs), np.int8)
    for s in range(64):
        reg, v = s, []
        for u in rng.integers(0, 2, Cs // 2).tolist():
            reg, v0, v1 = ML.register_step(reg, u)
            v += [v0, v1]
        out[s, :len(v)] = X.hard_soft(v)
    return out


def spread(max_len, n):
    """n lengths from 0 to max_len, both included."""
    return sorted({int(v) for v in np.linspace(0, max_len, n)})


def short_batches(rng):
    """The shapes where a random header is rarely a valid length (h 2, and the
    minimal rows with max_len 5 and 3), so mostly planted frames: the h 2 row
    of max_len 24, the minimal row St = 8 h + 64 and the same with an odd soft
    count, for both header widths. Each with noise, weak, zero and negated rows
    beside the frames."""
    out = []
    shapes = [H2 + (n_soft(*H2),)]
    for h, kind in ((1, C.CRC16), (2, C.CRC32)):
        for Cs in (2 * (8 * h + 64), 2 * (8 * h + 64) + 1):
            shapes.append((h, kind, X.row_shape(1, Cs, h, kind)[2], Cs))
    for h, kind, max_len, Cs in shapes:
        lens = spread(max_len, 12)
        q = np.concatenate([planted(rng, lens + lens, h, kind, Cs, 40), planted(rng, lens[:4], h, kind, Cs, 25),
                            planted(rng, lens[-3:], h, kind, Cs, 12, erase=0.2), uniform(rng, 2, Cs),
                            weak(rng, 2, Cs), np.zeros((1, Cs), np.int8), negated(rng, lens[:2], h, kind, Cs)])
        out.append((h, kind, q))
    return out


def long_batch(rng, family):
    """7 or more rows of the 2070-step shape: the family's rows and one of zeros."""
    h, kind, max_len = LONG
    Cs = n_soft(*LONG)
    lens = spread(max_len, 6)
    if family == "uniform":
        q = uniform(rng, 6, Cs)
    elif family == "weak":
        q = weak(rng, 6, Cs)
    elif family == "negated":
        q = negated(rng, lens, h, kind, Cs)
    elif family == "other-starts":
        q = other_starts(rng, Cs)
    else:
        a = int(family.split("-")[1])
        q = planted(rng, lens, h, kind, Cs, a, erase=0.2 if a == 12 else 0.0)
    return h, kind, np.concatenate([q, np.zeros((1, Cs), np.int8)])


FAMILIES = ("uniform", "weak", "planted-40", "planted-25", "planted-12", "negated", "other-starts")
CASES = FAMILIES + ("short",)


def case_batches(case):
    """[(h, kind, q [n][C])] of one parametrised case, seeded by its name alone."""
    rng = np.random.default_rng(1 + CASES.index(case))
    return short_batches(rng) if case == "short" else [long_batch(rng, case)]


def fixture_holds(case, batches, oks, steps):
    """The conditions that keep the row check from passing on nothing: at
    least half the case's rows are OK, every row where every header is valid,
    and the OK rows' steps take 4 values or more. (A minimal row has one
    possible T, the all-zero row one possible verdict: they ride in cases
    with other rows.)"""
    ok, st = np.concatenate(oks), np.concatenate(steps)
    assert 2 * int(ok.sum()) >= ok.size, (case, int(ok.sum()), ok.size)
    for (h, kind, q), o in zip(batches, oks):
        if (h, kind, q.shape[1]) == LONG[:2] + (n_soft(*LONG),):
            assert o.all(), case
    assert len(set(st[ok].tolist())) >= 4, (case, sorted(set(st[ok].tolist())))


def host_decode(A, q, h, kind):
    out = [A.coded_frame_decode(row, h, kind) for row in q]
    return [o[0] for o in out], ML.records([o[1] for o in out])


# ---- a. the reference against enumeration ------------------------------------------------

@pytest.mark.parametrize("T", range(1, 13))
def test_reference_against_enumeration(T):
    """All 2^T inputs through a plain shift-register loop against best():
    free, into state 0 (T >= 6: six inputs flush the register), into another
    state, and behind a fixed prefix. Soft values from the whole int8 range,
    from {-2 .. 2} (ties) and with a third set to zero."""
    rng = np.random.default_rng(T)
    rows = [rng.integers(-128, 128, 2 * T), rng.integers(-2, 3, 2 * T), np.zeros(2 * T, np.int64),
            np.where(rng.random(2 * T) < 0.33, 0, rng.integers(-128, 128, 2 * T))]
    q = np.array(rows, np.int64)
    prefix = tuple(rng.integers(0, 2, min(T, 3)).tolist())
    wants = [(dict(), [ML.enumerate_best(r, T) for r in q]),
             (dict(fixed=prefix), [ML.enumerate_best(r, T, fixed=prefix) for r in q])]
    if T >= 6:
        for end in (0, 37):
            wants.append((dict(end=end), [ML.enumerate_best(r, T, end=end) for r in q]))
        wants.append((dict(fixed=prefix, end=0), [ML.enumerate_best(r, T, fixed=prefix, end=0) for r in q]))
    for kw, want in wants:
        assert ML.best(q, T, **kw).tolist() == want, (T, kw)
        assert int(ML.best(q[0], T, **kw)) == want[0]
    # one T a row, a fixed bit a row with free ones between: the forms check_decodes uses
    Ts = np.array([T, max(T - 1, 0), T, 0])
    fixed = np.array([[1, -1, 0], [-1, -1, -1], [0, 0, 0], [1, 1, 1]])[:, :min(T, 3)]
    got = ML.best(q, Ts, fixed=fixed)
    for r in range(4):
        t, f = int(Ts[r]), fixed[r, :int(Ts[r])].tolist()
        full = [p for p in np.ndindex(*(2,) * len(f)) if all(x in (-1, b) for x, b in zip(f, p))]
        assert int(got[r]) == max(ML.enumerate_best(q[r], t, fixed=p) for p in full), (T, r)
    if T < 6:                                        # no path of T < 6 steps from state 0 ends in state 32
        assert (ML.best(q, T, end=32) == ML.UNREACHABLE).all()


# ---- b. the code is the code ----------------------------------------------------------------

def test_table_is_the_encoder():
    """A walk of the transition table gives frames_fec_ref.encode_bits' bits
    (which tests/test_frames_fec_cpu.py::test_encoder holds equal to the
    library's): this pins the register's orientation, which the spectrum
    cannot (the time-reversed generators have the same one)."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 9, 40, 300):
        info = rng.integers(0, 256, n).astype(np.uint8).tobytes()
        T = 8 * n + 6
        u = np.concatenate([np.unpackbits(np.frombuffer(info, np.uint8)), np.zeros(6, np.uint8)])
        assert np.array_equal(ML.walk(u), X.encode_bits(info, T)), n
    assert (ML.G0, ML.G1) == (X.G0, X.G1) == (0o171, 0o133)
    src = open(os.path.join(ROOT, "include", "demod.h")).read()
    assert "parity(reg_t & 0171)" in src and "parity(reg_t & 0133)" in src and "((reg_t-1 << 1) | u_t)" in src


def test_first_event_weight_spectrum():
    """The published spectrum of the K = 7, rate-1/2 code 171/133: free
    distance 10; 11, 38 and 193 first-event paths of weight 10, 12 and 14
    carrying 36, 211 and 1404 information bits; none of odd weight."""
    assert ML.first_event_spectrum(15) == {10: (11, 36), 12: (38, 211), 14: (193, 1404)}


# ---- c. the decoders are maximum-likelihood ----------------------------------------------------

@pytest.fixture(scope="module")
def batches():
    return {case: case_batches(case) for case in CASES}


@pytest.mark.parametrize("who", ["host", "numpy"])
@pytest.mark.parametrize("case", CASES)
def test_decoders_are_maximum_likelihood(A, batches, case, who):
    """fec_ml_ref.check_decodes on every row of the case, for the library's
    demod_coded_frame_decode and for frames_fec_ref.decode_rows."""
    oks, steps = [], []
    for h, kind, q in batches[case]:
        written, dec = host_decode(A, q, h, kind) if who == "host" else X.decode_rows(q, h, kind)
        ok, st = ML.check_decodes(q, h, C.CRC_BYTES[kind], written, dec, (who, case, h, q.shape[1]))
        oks.append(ok)
        steps.append(st)
    fixture_holds(case, batches[case], oks, steps)


def test_host_decoder_takes_minus_128(A):
    """-128 is no soft value the library makes, but the host decoder takes any
    int8: its verdicts are still maximum-likelihood."""
    rng = np.random.default_rng(128)
    h, kind, _ = LONG
    q = uniform(rng, 6, n_soft(*LONG), low=-128)
    q[0] = -128
    assert (q == -128).sum() > 4000
    written, dec = host_decode(A, q, h, kind)
    ok, st = ML.check_decodes(q, h, C.CRC_BYTES[kind], written, dec, "host")
    assert ok.all() and len(set(st.tolist())) >= 4


def longest_negated(rng):
    """Family 5 at the longest row (max_len 4096, h 2, CRC-32: 32822 steps):
    the negated +-127 codeword of the complement of a 4095-byte frame's
    information bits (ones behind them). Both generators have an odd number
    of taps, so that the best path is the frame itself behind a disturbed
    start and its header a valid length: the row is decoded over
    LONGEST_NEGATED_STEPS of its 32822 steps. (The disturbed start never
    decodes to a length whose high byte is 0x10: no choice of the first 16
    inputs gives 4096, 4095 is the longest.) The disturbed start also leaves
    two best headers, 0x0FFF and 0x3FFF; the first value on which their
    codewords differ and that speaks against the frame is inverted, so that
    the row's verdict does not hang on the decoder's tie rule. Returns (q int8
    [C], h, kind)."""
    h, kind = 2, C.CRC32
    Cs = Z.symbols_for(4096, 1, h, kind, X.CONV_K7)
    info = C.encode(rng.integers(0, 256, 4095).astype(np.uint8).tobytes(), h, kind)
    T = Cs // 2
    q = -X.hard_soft(X.encode_bits(bytes(b ^ 0xFF for b in info) + b"\xff" * ((T + 7) // 8 - len(info)), T))
    own, other = (X.hard_soft(X.encode_bits(head + info[2:12], 80)) for head in (info[:2], b"\x3f\xff"))
    at = np.flatnonzero((own != other) & (q[:160] != own))[0]
    q[at] = -q[at]
    return q, h, kind


LONGEST_NEGATED_STEPS = 8 * (2 + 4095 + 4) + 6


def test_longest_row_negated_codeword(A):
    q, h, kind = longest_negated(np.random.default_rng(4096))
    assert q.size == 2 * 32822 and set(np.unique(q).tolist()) == {-127, 127}
    for who, (written, dec) in (("host", host_decode(A, q[None], h, kind)), ("numpy", X.decode_rows(q[None], h, kind))):
        ok, st = ML.check_decodes(q[None], h, C.CRC_BYTES[kind], written, dec, who)
        assert ok.all() and st.tolist() == [LONGEST_NEGATED_STEPS] and dec["metric"][0] > 250 * st[0], who


# ---- d. the metric floor -----------------------------------------------------------------------

def header_constant(name):
    src = open(os.path.join(ROOT, "include", "demod.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))


def test_metric_floor_is_safe(A):
    """The decoders start the states other than 0 at -2^28 where the reference
    has "unreachable". Two bounds make that the same thing, both from the
    header's constants: the longest row's metrics stay inside int32 around the
    floor (254 St_max < 2^28, and with the host's -128: 256 St_max), and a
    path from another state cannot catch up (it differs from the path of the
    same inputs from state 0 in its first 6 steps alone, by 2 (|q0| + |q1|) <=
    512 a step). Raising the payload limit trips this test."""
    payload, depth = header_constant("DEMOD_MAX_FRAME_PAYLOAD"), header_constant("DEMOD_FEC_DEPTH")
    assert payload == A.DEMOD_MAX_FRAME_PAYLOAD and depth == A.DEMOD_FEC_DEPTH == ML.DEPTH
    st_max = max(8 * (2 + payload + 4) + 6, 8 * 2 + depth)
    assert st_max == A.coded_frame_steps(payload, 2, C.CRC32) == 32822
    assert 254 * st_max < 2 ** 28
    assert 2 ** 28 + 256 * st_max < 2 ** 31
    assert 6 * 2 * (128 + 128) < 2 ** 28
    with pytest.raises(A.DemodError):                        # and no longer row is taken
        A.coded_frame_decode(np.zeros(2 * (st_max + 8), np.int8), 2, C.CRC32, cap=8192)


# ---- e. the soft values agree with the hard decision -----------------------------------------------

@pytest.mark.parametrize("K", [2, 4, 8, 16])
def test_soft_values_agree_with_the_hard_decision(A, K):
    """The decoder never reads the hard symbols. For finite powers with one
    greatest tone, soft value b is >= 0 where bit b (MSB first) of that tone
    is clear and <= 0 where it is set."""
    rng = np.random.default_rng(K)
    bits = K.bit_length() - 1
    P = np.concatenate([rng.exponential(1.0, (300, K)), rng.integers(0, 50, (300, K)), rng.normal(0.0, 1.0, (200, K)),
                        -rng.exponential(1.0, (50, K)), rng.random((50, K)) * 1e-38, rng.random((50, K)) * 3e38,
                        1000.0 + rng.integers(0, 3, (100, K))]).astype(np.float32)
    P = P[(P == P.max(axis=1, keepdims=True)).sum(axis=1) == 1]
    assert len(P) > 700 and np.isfinite(P).all()
    seen = set()
    for row in P:
        q, top = A.soft_bits(row), int(np.argmax(row))
        for b in range(bits):
            if (top >> (bits - 1 - b)) & 1:
                assert q[b] <= 0, (row, b, q)
            else:
                assert q[b] >= 0, (row, b, q)
        seen |= {int(np.sign(v)) for v in q}
    assert seen == {-1, 0, 1}
