"""Coded frames on the GPU (frames_fec.hip, the coded check of frames_check.hip)
against tests/frames_fec_ref.py.

Kernel level: test-made hits, results, tables and powers on the device, so no
detector and no scan run. d_rows, d_decode and d_work are poisoned; rows and
decode are compared WHOLE with the reference laid over the same poison: one
comparison says that what must be written is written, bit for bit, and that
nothing else is. What a row decodes to is always the reference's verdict on
the same powers.

End to end: five coded frames as 2-FSK and 8-FSK PCM, three of them with three
payload symbols replaced by a wrong tone, through demod_frames_coded and, as
two segments, through the segmented scan, the decode and the coded check.
"""
import ctypes
import functools

import numpy as np
import pytest

import fec_modes_ref as Z
import frames_check_ref as C
import frames_fec_ref as X
import frames_ref as F
import guards as G
from gpu_support import handle_fixture, phased, results_bytes, same as whole_same, tones_375, torch  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPE_OF_R = {1: (1024, 1024), 4: (1024, 256), 64: (512, 8)}    # (n, hop) of a handle with R phases
RES_BYTES = F.RESULT_DTYPE.itemsize
LEAD = 4096          # guard bytes per side (a multiple of 8)
POISON = 0xFF
L0 = 8               # the word's symbols in the kernel-level tests (it is never read)


# handle(R, K): one Demodulator per (R, K), closed with the module.
handle = handle_fixture(lambda A, Rn, K: phased(A, SHAPE_OF_R, Rn, tones_375(K)))


def min_symbols(bits, h):
    """The smallest N a call accepts: St = 8 h + 64."""
    return (2 * (8 * h + X.DEPTH) + bits - 1) // bits


def info_symbols(info, T, N, bits, rng, flips=4):
    """N symbols: the 2 T coded bits of the information bytes `info` with
    `flips` of them inverted (cut at the row's end), random bits behind."""
    coded = X.encode_bits(info, T)
    if flips:
        coded[rng.choice(min(coded.size, N * bits), flips, replace=False)] ^= 1
    b = np.concatenate([coded, rng.integers(0, 2, max(0, N * bits - coded.size)).astype(np.uint8)])[:N * bits]
    return (b.reshape(N, bits) << np.arange(bits - 1, -1, -1, dtype=np.uint8)).sum(axis=1).astype(np.uint8)


def frame_symbols(rng, length, N, bits, h, kind, flips=4):
    """A coded frame of `length` random data bytes as N row symbols, and its checked frame."""
    frame = C.encode(rng.integers(0, 256, length).astype(np.uint8).tobytes(), h, kind)
    return info_symbols(frame, X.steps(length, h, kind), N, bits, rng, flips), frame


def powers_for(sym, K, rng):
    """P float32 [W][K]: the symbol's tone 1000 .. 1999, the others 1 .. 299."""
    P = rng.integers(1, 300, (sym.size, K)).astype(np.float32)
    P[np.arange(sym.size), sym] = rng.integers(1000, 2000, sym.size)
    return P


def lay_rows(rows_sym, K, Rn, rng, L=L0, lead=3):
    """The rows' symbols laid one behind the other on phase `lead` % R, symbol
    j of row r at window start_r + (L + j) R; random symbols everywhere else.
    Returns (P [W][K], start windows)."""
    N = len(rows_sym[0])
    span = (L + N) * Rn
    W = lead + len(rows_sym) * span + 5
    sym = rng.integers(0, K, W).astype(np.uint8)
    starts = []
    for r, row in enumerate(rows_sym):
        s = lead + r * span
        sym[s + L * Rn:s + (L + N) * Rn:Rn] = row
        starts.append(s)
    return powers_for(sym, K, rng), np.array(starts, np.uint64)


def reference(P, n_windows, first, hits, n_written, L, Rn, N, h, kind, poison=POISON, decoder=None):
    """rows [G][max_frames][Bd] and decode [G][max_frames][16] whole: the
    reference laid over poison. Rows with the same absolute start decode once."""
    n_groups, max_frames = hits.shape
    K = P.shape[1]
    bits = F.bits_per_symbol(K)
    St, Bd, max_len = X.row_shape(N, bits, h, kind)
    rows = np.full((n_groups, max_frames, Bd), poison, np.uint8)
    dec = np.full((n_groups, max_frames, 16), poison, np.uint8)
    soft = X.soft_bits(P[:n_windows])
    keys, where = {}, []
    for g in range(n_groups):
        base = 0 if first is None else min(int(first[g]), n_windows)
        for i in range(min(int(n_written[g]), max_frames)):
            w = int(hits["window"][g, i])
            key = (base, w) if w < n_windows else None
            keys.setdefault(key, X.row_soft(soft, n_windows, base, w, L, Rn, N))
            where.append((g, i, key))
    if not where:
        return rows, dec, {}
    order = list(keys)
    if decoder is None:
        written, d = X.decode_rows(np.array([keys[k] for k in order]), h, kind)
    else:
        out = [decoder(keys[k], h, kind) for k in order]
        written = [o[0] for o in out]
        d = np.array([tuple(o[1][f] for f in X.DECODE_DTYPE.names) for o in out], X.DECODE_DTYPE)
    at = {k: n for n, k in enumerate(order)}
    for g, i, key in where:
        n = at[key]
        rows[g, i, :len(written[n])] = np.frombuffer(written[n], np.uint8)
        dec[g, i] = d[n:n + 1].view(np.uint8)
    return rows, dec, {k: (written[at[k]], d[at[k]]) for k in order}


class Run:
    """One decode call on test-made inputs; rows, decode and the workspace
    poisoned (with guard: between poisoned guard bands)."""

    def __init__(self, A, torch, P, hits, n_written, first=None, n_windows=None, poison=POISON, guard=False,
                 work_poison=None):
        self.A, self.torch = A, torch
        self.n_groups, self.max_frames = hits.shape
        self.W = P.shape[0] if n_windows is None else n_windows
        self.inputs = [np.ascontiguousarray(hits).view(np.uint8).reshape(-1),
                       np.ascontiguousarray(P, np.float32).reshape(-1), results_bytes(n_written).reshape(-1)]
        if first is not None:
            self.inputs.append(np.array([int(f) for f in first], "<u8").view(np.int64))
        self.d_in = [torch.from_numpy(a.copy()).cuda() for a in self.inputs]
        self.poison, self.guard = poison, guard
        self.work_poison = poison if work_poison is None else work_poison
        self.checks = []

    def out(self, nbytes, poison):
        torch = self.torch
        if not self.guard:
            return torch.full((nbytes,), poison, dtype=torch.uint8, device="cuda")
        t, chk = G.guarded(torch, nbytes, torch.uint8, LEAD, LEAD, poison)
        self.checks.append(chk)
        return t

    def __call__(self, d, L, N, h, kind, stream=0):
        torch = self.torch
        rows = self.n_groups * self.max_frames
        Bd = X.row_shape(N, F.bits_per_symbol(d.k), h, kind)[1]
        self.d_rows, self.d_dec = self.out(rows * Bd, self.poison), self.out(rows * 16, self.poison)
        work = self.out(self.A.frames_decode_workspace_size(d.cfg, self.n_groups, self.max_frames, N),
                        self.work_poison)
        d.frames_decode_async(self.d_in[0], self.d_in[1], self.W, self.d_in[3] if len(self.d_in) > 3 else None,
                              self.d_in[2], self.n_groups, self.max_frames, L, N, h, kind, self.d_rows, self.d_dec,
                              work, stream=stream)
        torch.cuda.synchronize()
        for chk in self.checks:
            chk(written=False)
        for t, a in zip(self.d_in, self.inputs):
            assert t.cpu().numpy().tobytes() == a.tobytes(), "an input was written to"     # NaNs compare as bytes
        return (self.d_rows.cpu().numpy().reshape(self.n_groups, self.max_frames, Bd),
                self.d_dec.cpu().numpy().reshape(self.n_groups, self.max_frames, 16))


same = functools.partial(whole_same, names=("rows", "decode"))


def one_group(starts, max_frames=None):
    hits = np.zeros((1, max_frames or len(starts)), C.HIT_DTYPE)
    hits["window"][0, :len(starts)] = starts
    return hits


def edge_lengths(max_len, h, kind):
    """0, 1, the lengths on either side of 8 n + 6 = 8 h + 64, max_len."""
    c = C.CRC_BYTES[kind]
    return sorted({n for n in (0, 1, 7 - c, 8 - c, max_len) if 0 <= n <= max_len})


def shape_rows(rng, N, bits, h, kind, K):
    """The rows of one shape: the edge lengths with 4 flipped coded bits each,
    a header of max_len + 1, a header of all ones, a row of random symbols."""
    St, Bd, max_len = X.row_shape(N, bits, h, kind)
    rows, frames = [], []
    for n in edge_lengths(max_len, h, kind):
        row, frame = frame_symbols(rng, n, N, bits, h, kind)
        rows.append(row)
        frames.append(frame)
    for info in ((max_len + 1).to_bytes(h, "big"), b"\xff" * h):
        rows.append(info_symbols(info + rng.integers(0, 256, Bd).astype(np.uint8).tobytes(), St, N, bits, rng, 0))
    rows.append(rng.integers(0, K, N).astype(np.uint8))
    return rows, frames


def spoil(P, starts, Rn, N, rng):
    """Windows of the last row with equal, zero, negative, NaN and Inf powers."""
    K = P.shape[1]
    w = int(starts[-1]) + (L0 + np.arange(N)) * Rn
    P[w[0]] = 7.0
    P[w[1]] = 0.0
    P[w[2]] = -rng.integers(1, 300, K).astype(np.float32)
    P[w[3], rng.integers(0, K)] = np.nan
    P[w[4]] = np.nan
    P[w[5], rng.integers(0, K)] = np.inf
    P[w[6]] = np.inf
    P[w[7], 0] = -np.inf
    P[w[8], K - 1] = 3.0e38


# ---- shapes -----------------------------------------------------------------------

@pytest.mark.parametrize("kind", [C.CRC16, C.CRC32])
@pytest.mark.parametrize("h", [1, 2])
@pytest.mark.parametrize("Rn", [1, 4, 64])
@pytest.mark.parametrize("K", [2, 4, 8, 16])
def test_shapes(A, torch, handle, K, Rn, h, kind):
    """The minimal N, the next N (an odd C at 1 and 3 bits; at 3 bits step
    pairs straddle symbols) and a row of max_len 24: the edge lengths, each
    frame with 4 flipped coded bits and random symbols behind it, a header of
    max_len + 1 and of all ones, and a random row holding equal, zero,
    negative, NaN and Inf powers. The planted frames come back exactly."""
    d = handle(Rn, K)
    bits = F.bits_per_symbol(K)
    n0 = min_symbols(bits, h)
    statuses = set()
    for N in (n0, n0 + 1, Z.symbols_for(24, bits, h, kind, X.CONV_K7)):
        rng = np.random.default_rng(N * 1000 + K * 10 + h + kind)
        rows, frames = shape_rows(rng, N, bits, h, kind, K)
        P, starts = lay_rows(rows, K, Rn, rng)
        spoil(P, starts, Rn, N, rng)
        hits = one_group(starts, len(starts) + 2)
        want = reference(P, len(P), None, hits, [len(starts)], L0, Rn, N, h, kind)
        got = Run(A, torch, P, hits, [len(starts)])(d, L0, N, h, kind)
        same(got, want[:2], (K, Rn, N))
        for i, frame in enumerate(frames):          # the fixture's condition: 4 flips are corrected
            written, dec = want[2][0, int(starts[i])]
            assert written == frame and dec["status"] == X.OK, (N, i)
        statuses |= {int(v[1]["status"]) for v in want[2].values()}
    assert statuses == {X.OK, X.BAD_LENGTH}


def test_longest_row(A, torch, handle):
    """One row of max_len 4096 (h 2, CRC-32, 16 tones: 32822 steps), against
    the host decoder demod_coded_frame_decode on the reference's soft values
    (tests/test_frames_fec_cpu.py holds that decoder to the reference)."""
    K, Rn, h, kind, bits = 16, 1, 2, C.CRC32, 4
    N = Z.symbols_for(4096, bits, h, kind, X.CONV_K7)
    assert X.row_shape(N, bits, h, kind)[2] == 4096
    rng = np.random.default_rng(4096)
    row, frame = frame_symbols(rng, 4096, N, bits, h, kind, flips=0)
    for at in range(100, N - 100, 997):             # a wrong tone now and then
        row[at] ^= 5
    P, starts = lay_rows([row], K, Rn, rng)
    hits = one_group(starts)
    want = reference(P, len(P), None, hits, [1], L0, Rn, N, h, kind, decoder=A.coded_frame_decode)
    assert want[2][0, int(starts[0])][0] == frame
    same(Run(A, torch, P, hits, [1])(handle(Rn, K), L0, N, h, kind), want[:2])


# ---- counts, groups, erasures -------------------------------------------------------

def pool(rng, K, Rn, h, kind, N, count=24):
    """`count` rows of one shape (frames of drawn lengths, every fourth a
    random row) laid in one batch: (P, starts)."""
    bits = F.bits_per_symbol(K)
    max_len = X.row_shape(N, bits, h, kind)[2]
    rows = [rng.integers(0, K, N).astype(np.uint8) if r % 4 == 3 else
            frame_symbols(rng, int(rng.integers(0, max_len + 1)), N, bits, h, kind)[0] for r in range(count)]
    return lay_rows(rows, K, Rn, rng)


def test_counts_and_erasures(A, torch, handle):
    """Groups of 0, 1, 63, 64 and 65 rows and two whose stored n_written is
    above max_frames; hits whose frame runs past n_windows at every symbol
    count from 0 (erasures, nothing read past the powers), a hit at
    n_windows and beyond, and one of 2^64 - 1."""
    K, Rn, h, kind = 4, 4, 1, C.CRC16
    d = handle(Rn, K)
    N = Z.symbols_for(9, 2, h, kind, X.CONV_K7)
    rng = np.random.default_rng(77)
    P, starts = pool(rng, K, Rn, h, kind, N)
    W = len(P)
    max_frames = 65
    counts = [0, 1, 63, 64, 65, max_frames + 7, 2 ** 64 - 1]
    hits = np.zeros((len(counts), max_frames), C.HIT_DTYPE)
    hits["window"] = starts[rng.integers(0, len(starts), hits.shape)]
    late = [W - (L0 + j) * Rn - 1 for j in range(0, N + 1, 5)] + [W - 1, W, W + 1, 2 ** 31, 2 ** 63, 2 ** 64 - 1]
    hits["window"][4, :len(late)] = np.array(late, np.uint64)
    hits["window"][6, 5:9] = np.array([W - 2, W, 2 ** 40, 2 ** 64 - Rn * (L0 + 3)], np.uint64)
    want = reference(P, W, None, hits, counts, L0, Rn, N, h, kind)
    same(Run(A, torch, P, hits, counts)(d, L0, N, h, kind), want[:2])
    # fewer windows than the allocation holds: the rows that leave the batch change, none faults
    W2 = W - 3 * (L0 + N) * Rn - 7
    want2 = reference(P, W2, None, hits, counts, L0, Rn, N, h, kind)
    same(Run(A, torch, P, hits, counts, n_windows=W2)(d, L0, N, h, kind), want2[:2])
    assert not np.array_equal(want[0], want2[0])


def test_more_rows_than_waves(A, torch, handle):
    """1024 groups x 32 minimal rows: 16 waves a group, each takes two rows
    and reuses its workspace slot. The workspace is poisoned before each call,
    with two poisons: no word is read before the call wrote it."""
    K, Rn, h, kind = 2, 1, 1, C.CRC16
    d = handle(Rn, K)
    N = min_symbols(1, h)
    rng = np.random.default_rng(1024)
    P, starts = pool(rng, K, Rn, h, kind, N, count=64)
    hits = np.zeros((1024, 32), C.HIT_DTYPE)
    hits["window"] = starts[rng.integers(0, len(starts), hits.shape)]
    counts = rng.integers(0, 33, 1024).tolist()
    counts[0], counts[1], counts[-1] = 32, 0, 32
    want = reference(P, len(P), None, hits, counts, L0, Rn, N, h, kind)
    for work_poison in (0xFF, 0x00):
        same(Run(A, torch, P, hits, counts, work_poison=work_poison)(d, L0, N, h, kind), want[:2], work_poison)


# ---- segments ------------------------------------------------------------------------

def test_segments(A, torch, handle):
    """With a segment table a hit's window is relative to min(first[g],
    n_windows): the same rows under two different first[] and in another slot
    give identical bytes, and a first[] above n_windows is clamped (every value
    an erasure)."""
    K, Rn, h, kind = 8, 4, 2, C.CRC16
    d = handle(Rn, K)
    N = Z.symbols_for(6, 3, h, kind, X.CONV_K7)
    rng = np.random.default_rng(8)
    P, starts = pool(rng, K, Rn, h, kind, N, count=10)
    W = len(P)
    shift = 3 * (L0 + N) * Rn
    tail = np.concatenate([P[shift:], P[:shift]])              # the same rows, `shift` windows earlier
    both = np.concatenate([P, tail])
    rel = starts[3:8] - np.uint64(shift)
    hits = np.zeros((4, 6), C.HIT_DTYPE)
    hits["window"][0, :5] = rel
    hits["window"][1, :5] = starts[:5]
    hits["window"][2, :5] = rel
    hits["window"][3, :5] = starts[:5]
    first = [shift, 0, W, 2 ** 64 - 1]
    counts = [5, 5, 5, 3]
    want = reference(both, 2 * W, first, hits, counts, L0, Rn, N, h, kind)
    got = Run(A, torch, both, hits, counts, first=first)(d, L0, N, h, kind)
    same(got, want[:2])
    for a in got:
        assert np.array_equal(a[0], a[2])                      # another first[], another slot
    zero = X.decode(np.zeros(N * 3, np.int8), h, kind)
    assert bytes(got[0][3, 0, :len(zero[0])]) == zero[0] and got[1][3, 0].tobytes() == zero[1].tobytes()


# ---- guards ----------------------------------------------------------------------------

@pytest.mark.parametrize("Rn,K,h,kind", [(4, 2, 1, C.CRC16), (1, 16, 2, C.CRC32), (64, 8, 2, C.CRC16)])
def test_guards(A, torch, handle, Rn, K, h, kind):
    """d_rows, d_decode and d_work between poisoned guards, two poisons: the
    guards and every byte the contract does not list keep the poison, every
    listed byte is written (it equals the reference under both poisons), the
    inputs are unchanged."""
    d = handle(Rn, K)
    bits = F.bits_per_symbol(K)
    N = Z.symbols_for(11, bits, h, kind, X.CONV_K7) + 1
    rng = np.random.default_rng(K + Rn)
    P, starts = pool(rng, K, Rn, h, kind, N)
    counts, max_frames = [40, 0, 70], 70
    hits = np.zeros((3, max_frames), C.HIT_DTYPE)
    hits["window"] = starts[rng.integers(0, len(starts), hits.shape)]
    hits["window"][2, 69] = len(P) - 3
    for poison in (0xFF, 0x5A):
        want = reference(P, len(P), None, hits, counts, L0, Rn, N, h, kind, poison)
        same(Run(A, torch, P, hits, counts, poison=poison, guard=True)(d, L0, N, h, kind), want[:2], poison)


# ---- refusals ---------------------------------------------------------------------------

def test_refusals(A, torch, handle):
    """Every DEMOD_BAD_ARG case of the two device entries returns without a
    launch: the outputs stay poison."""
    lib = A.load_library()
    d = handle(4, 2)
    S, cap, N, L, W = 3, 16, 200, 8, 5000             # St 100, Bd 11
    rows = S * cap
    u8 = dict(dtype=torch.uint8, device="cuda")

    def poison(nbytes):
        return torch.full((nbytes,), 0xFF, **u8)
    d_hits = torch.zeros(rows * 16 + 8, **u8)
    d_mag = torch.ones(W * 2, dtype=torch.float32, device="cuda")
    d_first = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(S * RES_BYTES + 8, **u8)
    need = A.frames_decode_workspace_size(d.cfg, S, cap, N)
    assert need == S * cap * 100 * 8
    d_rows, d_dec, d_work = poison(rows * 11), poison(rows * 16 + 8), poison(need + 8)
    d_check, d_kept, d_body, d_sum = poison(rows * 16 + 8), poison(rows * 4 + 8), poison(rows * 8), poison(S * 32 + 8)
    ph, pm, pf, pr, po, pd, pw = (t.data_ptr() for t in (d_hits, d_mag, d_first, d_res, d_rows, d_dec, d_work))
    pc, pk, pb, ps = (t.data_ptr() for t in (d_check, d_kept, d_body, d_sum))

    def decode(h=d._h, hits=ph, mag=pm, n_windows=W, first=None, res=pr, n_groups=S, max_frames=cap, sync_len=L,
               n=N, len_bytes=1, crc=A.DEMOD_CRC16_CCITT_FALSE, fec=1, out=po, dec=pd, work=pw, work_bytes=need):
        return lib.demod_frames_decode_async(h, hits, mag, n_windows, first, res, n_groups, max_frames, sync_len,
                                             n, len_bytes, crc, fec, out, dec, work, work_bytes, None)

    def check(h=d._h, hits=ph, packed=po, res=pr, n_groups=S, max_frames=cap, sync_len=L, n=N, len_bytes=1,
              crc=A.DEMOD_CRC16_CCITT_FALSE, fec=1, chk=pc, kept=pk, body=pb, summ=ps):
        return lib.demod_frames_check_coded_async(h, hits, packed, res, n_groups, max_frames, sync_len, n,
                                                  len_bytes, crc, fec, chk, kept, body, summ, None)

    shared = dict([
        ("NULL handle", dict(h=None)),
        ("NULL d_hits", dict(hits=None)),
        ("NULL d_results", dict(res=None)),
        ("misaligned d_hits", dict(hits=ph + 4)),
        ("misaligned d_results", dict(res=pr + 4)),
        ("n_groups == 0", dict(n_groups=0)),
        ("n_groups > DEMOD_MAX_SEGMENTS", dict(n_groups=A.DEMOD_MAX_SEGMENTS + 1, max_frames=1)),
        ("n_groups * max_frames >= 2^31", dict(n_groups=2 ** 15, max_frames=2 ** 16)),
        ("max_frames >= 2^31", dict(n_groups=1, max_frames=2 ** 31)),
        ("max_frames == 0", dict(max_frames=0)),
        ("sync_len == 0", dict(sync_len=0)),
        ("sync_len > DEMOD_MAX_SYNC", dict(sync_len=A.DEMOD_MAX_SYNC + 1)),
        ("len_bytes 0", dict(len_bytes=0)),
        ("len_bytes 3", dict(len_bytes=3)),
        ("crc 0", dict(crc=0)),
        ("crc 3", dict(crc=3)),
        ("fec 0", dict(fec=0)),
        ("fec 2", dict(fec=2)),
        ("St < 8 h + 64", dict(n=143)),
        ("St < 8 h + 64, h 2", dict(n=159, len_bytes=2)),
        ("frame_symbols == 0", dict(n=0)),
        ("max_len > DEMOD_MAX_FRAME_PAYLOAD", dict(n=2 * (8 * (4097 + 3) + 6), n_groups=1, max_frames=1)),
        ("frame_symbols >= 2^31", dict(n=2 ** 31)),
    ])
    for what, kw in shared.items():
        assert decode(**kw) == A.DEMOD_BAD_ARG, what
        assert check(**kw) == A.DEMOD_BAD_ARG, what
    for what, kw in dict([
        ("NULL d_mags", dict(mag=None)), ("NULL d_rows", dict(out=None)), ("NULL d_decode", dict(dec=None)),
        ("NULL d_work", dict(work=None)), ("misaligned d_decode", dict(dec=pd + 2)),
        ("misaligned d_work", dict(work=pw + 4)), ("misaligned d_first", dict(first=pf + 4)),
        ("work_bytes short", dict(work_bytes=need - 1)), ("n_windows >= 2^31", dict(n_windows=2 ** 31)),
        ("(L + N) R >= 2^31", dict(n=2 ** 29, n_groups=1, max_frames=1)),
    ]).items():
        assert decode(**kw) == A.DEMOD_BAD_ARG, what
    for what, kw in dict([
        ("NULL d_rows", dict(packed=None)), ("NULL d_check", dict(chk=None)), ("NULL d_kept", dict(kept=None)),
        ("NULL d_summary", dict(summ=None)), ("misaligned d_summary", dict(summ=ps + 4)),
        ("misaligned d_check", dict(chk=pc + 2)), ("misaligned d_kept", dict(kept=pk + 2)),
    ]).items():
        assert check(**kw) == A.DEMOD_BAD_ARG, what
    others = [A.Demodulator(n=1024, hop=384, freqs=(1500.0, 3000.0)),
              A.Demodulator(n=1024, hop=8, freqs=(1500.0, 3000.0)),
              A.Demodulator(n=1024, hop=256, freqs=tuple(1500.0 + 375.0 * i for i in range(5)))]
    try:
        for dd, what in zip(others, ("n % hop != 0", "R > 64", "K not a power of two")):
            assert decode(h=dd._h) == A.DEMOD_BAD_ARG, what
            assert check(h=dd._h) == A.DEMOD_BAD_ARG, what
        assert A.load_library().demod_frames_decode_workspace_size(ctypes.byref(others[2].cfg), S, cap, N) == 0
        with pytest.raises(A.DemodError):
            others[2].frames_coded(np.zeros(8192, np.int16), [0, 1], frame_symbols=400)
    finally:
        for dd in others:
            dd.close()
    # the Python mirror's own checks (before any pointer reaches the library)
    full = dict(d_hits=d_hits, d_mag=d_mag, d_first=None, d_results=d_res, d_rows=d_rows, d_decode=d_dec, d_work=d_work)
    for kw in (dict(d_hits=d_hits[:rows * 16 - 1]), dict(d_mag=d_mag[:W * 2 - 1]), dict(d_mag=d_mag.double()),
               dict(d_first=d_first[:S - 1]), dict(d_first=d_first.to(torch.int32)),
               dict(d_results=d_res[:S * RES_BYTES - 1]), dict(d_rows=d_rows[:rows * 11 - 1]),
               dict(d_decode=d_dec[:rows * 16 - 1]), dict(d_work=d_work[:need - 1]), dict(d_rows=None),
               dict(d_work=d_work.cpu())):
        a = dict(full)
        a.update(kw)
        with pytest.raises(A.DemodError) as e:
            d.frames_decode_async(a["d_hits"], a["d_mag"], W, a["d_first"], a["d_results"], S, cap, L, N, 1,
                                  A.DEMOD_CRC16_CCITT_FALSE, a["d_rows"], a["d_decode"], a["d_work"])
        assert e.value.code == A.DEMOD_BAD_ARG
    with pytest.raises(A.DemodError):
        d.frames_check_coded_async(d_hits, d_rows[:rows * 11 - 1], d_res, S, cap, L, N, 1, A.DEMOD_CRC16_CCITT_FALSE,
                                   d_check, d_kept[:rows * 4].view(torch.int32), d_body, d_sum)
    torch.cuda.synchronize()
    for t in (d_rows, d_dec, d_work, d_check, d_kept, d_body, d_sum):
        assert bool((t == 0xFF).all()), "a refused call wrote"
    # and the same calls, legal, run: three empty groups
    assert decode() == A.DEMOD_OK and decode(first=pf) == A.DEMOD_OK and check() == A.DEMOD_OK
    torch.cuda.synchronize()
    assert not d_sum[:S * 32].cpu().numpy().any()
    for t in (d_rows, d_dec, d_work, d_check, d_kept, d_body):
        assert bool((t == 0xFF).all())


# ---- a scan in front: determinism, capture and replay --------------------------------------

SCAN_R, SCAN_K, SCAN_L, SCAN_H, SCAN_KIND, SCAN_CAP = 4, 4, 16, 2, C.CRC16, 12
SCAN_N = Z.symbols_for(16, 2, SCAN_H, SCAN_KIND, X.CONV_K7)
SCAN_BD, SCAN_MAX = X.row_shape(SCAN_N, 2, SCAN_H, SCAN_KIND)[1:]


def scan_content(seed, n_frames, W=20001):
    """sym[W], P[W][4] and the word: n_frames coded frames on phase 1 among
    random symbols, each with 4 flipped coded bits; every third starts on the
    last 3 symbols (tail bits) of the one before: a covered frame."""
    rng = np.random.default_rng(seed)
    Rn, K, L, N = SCAN_R, SCAN_K, SCAN_L, SCAN_N
    word = np.random.default_rng(5).integers(0, K, L).astype(np.uint8)
    sym = rng.integers(0, K, W).astype(np.uint8)
    w, datas = 1 + 40 * Rn, []
    for f in range(n_frames):
        length = int(rng.integers(8, 17))
        # a frame whose last 3 symbols the next word overwrites has no flips of its own
        row, frame = frame_symbols(rng, length, N, 2, SCAN_H, SCAN_KIND, flips=0 if f % 3 == 1 else 4)
        sym[w:w + L * Rn:Rn] = word
        sym[w + L * Rn:w + (L + N) * Rn:Rn] = row
        datas.append(frame)
        Sc = X.coded_symbols(length, SCAN_H, SCAN_KIND, 2)
        # the next word behind this frame's plain span but inside its coded one, or well past the row
        w += (L + Sc - 3) * Rn if f % 3 == 1 else (L + N + 20 + int(rng.integers(0, 30))) * Rn
    assert w + (L + N) * Rn < W
    P = powers_for(sym, K, rng)
    P[1::Rn] *= np.float32(8.0)
    return sym, np.ascontiguousarray(P), word


def coded_expected(hits, rows, n_written, L, Rn, bits, h, kind, poison=POISON, fec=X.CONV_K7):
    """The check's four outputs whole, with the span of the mode `fec`."""
    n_groups, max_frames, Bd = rows.shape
    max_len = Bd - h - C.CRC_BYTES[kind]
    chk = np.full((n_groups, max_frames, 16), poison, np.uint8)
    kept = np.full((n_groups, max_frames, 4), poison, np.uint8)
    body = np.full((n_groups, max_frames, max_len), poison, np.uint8)
    summ = np.zeros(n_groups, C.SUMMARY_DTYPE)
    refs = []
    for g in range(n_groups):
        nw = min(int(n_written[g]), max_frames)
        r = C.check_group(hits["window"][g, :nw], rows[g, :nw], L, Rn, Z.span_of(bits, h, kind, fec), None, h, kind)
        chk[g, :nw] = r[0].view(np.uint8).reshape(-1, 16)
        kept[g, :len(r[1])] = r[1].view(np.uint8).reshape(-1, 4)
        for i, data in enumerate(r[2]):
            body[g, i, :len(data)] = np.frombuffer(data, np.uint8)
        summ[g] = r[3]
        refs.append(r)
    return dict(check=chk, kept=kept, body=body, summary=summ.view(np.uint8).reshape(n_groups, 32)), refs


def scan_reference(sym, P, word):
    hits, _, _, res = F.frames(sym, P, SCAN_R, word, 0, SCAN_N, max_frames=SCAN_CAP)
    nw = res["n_written"]
    h2 = np.zeros((1, SCAN_CAP), C.HIT_DTYPE)
    h2[0, :nw] = hits
    rows, dec, _ = reference(P, len(P), None, h2, [nw], SCAN_L, SCAN_R, SCAN_N, SCAN_H, SCAN_KIND)
    want, refs = coded_expected(h2, rows, [nw], SCAN_L, SCAN_R, 2, SCAN_H, SCAN_KIND)
    want.update(rows=rows, decode=dec)
    return res, want, refs[0]


class ScanBuffers:
    def __init__(self, A, torch, d, W):
        self.A, self.torch, self.d, self.W = A, torch, d, W
        u8 = dict(dtype=torch.uint8, device="cuda")
        self.d_sym = torch.zeros(W, **u8)
        self.d_P = torch.zeros((W, SCAN_K), dtype=torch.float32, device="cuda")
        self.d_work = torch.empty(A.frames_workspace_size(d.cfg, W), **u8)
        self.d_fwork = torch.empty(A.frames_decode_workspace_size(d.cfg, 1, SCAN_CAP, SCAN_N), **u8)
        self.d_hits, self.d_res = torch.empty(SCAN_CAP * 16, **u8), torch.empty(RES_BYTES, **u8)
        self.outs = dict(rows=torch.empty(SCAN_CAP * SCAN_BD, **u8), decode=torch.empty(SCAN_CAP * 16, **u8),
                         check=torch.empty(SCAN_CAP * 16, **u8), kept=torch.empty(SCAN_CAP * 4, **u8),
                         body=torch.empty(SCAN_CAP * SCAN_MAX, **u8), summary=torch.empty(32, **u8))

    def load(self, sym, P):
        self.d_sym.copy_(self.torch.from_numpy(sym))
        self.d_P.copy_(self.torch.from_numpy(P))

    def poison(self):
        for t in (self.d_hits, self.d_res, self.d_fwork, *self.outs.values()):
            t.fill_(POISON)

    def step(self, word, stream=0):
        o, d = self.outs, self.d
        d.frames_async(self.d_sym, self.d_P, self.W, word, 0, SCAN_N, self.d_hits, None, None, SCAN_CAP,
                       self.d_res, self.d_work, stream=stream)
        d.frames_decode_async(self.d_hits, self.d_P.view(-1), self.W, None, self.d_res, 1, SCAN_CAP, SCAN_L, SCAN_N,
                              SCAN_H, SCAN_KIND, o["rows"], o["decode"], self.d_fwork, stream=stream)
        d.frames_check_coded_async(self.d_hits, o["rows"], self.d_res, 1, SCAN_CAP, SCAN_L, SCAN_N, SCAN_H,
                                   SCAN_KIND, o["check"], o["kept"].view(self.torch.int32), o["body"],
                                   o["summary"], stream=stream)

    def results(self):
        self.torch.cuda.synchronize()
        shape = dict(rows=(1, SCAN_CAP, SCAN_BD), decode=(1, SCAN_CAP, 16), check=(1, SCAN_CAP, 16),
                     kept=(1, SCAN_CAP, 4), body=(1, SCAN_CAP, SCAN_MAX), summary=(1, 32))
        return {k: v.cpu().numpy().reshape(shape[k]) for k, v in self.outs.items()}


def test_determinism_and_second_stream(A, torch, handle):
    """Two runs, and a run on a second stream with buffers of its own, give
    byte-identical outputs: the reference's. Every third frame is covered
    under the coded span."""
    d = handle(SCAN_R, SCAN_K)
    sym, P, word = scan_content(3, 9)
    res, want, ref = scan_reference(sym, P, word)
    assert res["phase"] == 1 and res["n_hits"] >= 9 and 3 <= ref[3]["n_kept"] < ref[3]["n_valid"]
    a, b = ScanBuffers(A, torch, d, len(sym)), ScanBuffers(A, torch, d, len(sym))
    for buf in (a, b):
        buf.load(sym, P)
        buf.poison()
    runs = []
    a.step(word)
    runs.append(a.results())
    a.poison()
    a.step(word)
    runs.append(a.results())
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b.step(word, stream=side.cuda_stream)
    runs.append(b.results())
    for r in runs:
        same(r, want)


def test_capture_and_replay(A, torch, handle):
    """demod_frames_async + demod_frames_decode_async +
    demod_frames_check_coded_async in one graph on a side stream, replayed
    after the symbols and the powers were rewritten in place: each replay's
    bytes are the reference's for that content."""
    d = handle(SCAN_R, SCAN_K)
    contents = [scan_content(3, 9), scan_content(4, 5)]
    refs = [scan_reference(*c) for c in contents]
    assert int(refs[0][2][3]["n_kept"]) != int(refs[1][2][3]["n_kept"])
    buf = ScanBuffers(A, torch, d, len(contents[0][0]))
    word = contents[0][2]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        buf.load(*contents[0][:2])
        buf.poison()
        buf.step(word, stream=side.cuda_stream)          # an eager call of the shape first
        side.synchronize()
    same(buf.results(), refs[0][1], "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        buf.step(word, stream=torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        for (sym, P, _), (_, want, _) in zip(contents, refs):
            buf.load(sym, P)
            buf.poison()
            torch.cuda.synchronize()
            g.replay()
            same(buf.results(), want, rep)


# ---- the coded check -------------------------------------------------------------------------

@pytest.mark.parametrize("Rn,K", [(1, 2), (4, 8), (64, 16)])
def test_coded_check(A, torch, handle, Rn, K):
    """covered under the coded span on hand-made rows: a frame that starts on
    the window where the one before ends (touching: kept), one window earlier
    (covered), past the plain span but inside the coded one (covered only
    here), short frames whose span is the zero-filled 2 (8 h + 64) bits. And
    demod_frames_check_async on the same buffers still gives its old bytes."""
    d = handle(Rn, K)
    bits, h, kind, L = F.bits_per_symbol(K), 1, C.CRC16, 8
    N = Z.symbols_for(30, bits, h, kind, X.CONV_K7)
    Bd = X.row_shape(N, bits, h, kind)[1]
    B = (N * bits + 7) // 8
    rng = np.random.default_rng(Rn + K)
    lens = [30, 0, 3, 12, 5, 6, 30, 1, 20, 2, 9, 0]
    hits = np.zeros((1, len(lens) + 2), C.HIT_DTYPE)
    flat = rng.integers(0, 256, hits.size * B).astype(np.uint8)
    rows = flat.reshape(1, -1, B)                                # the scan's width: what the old entry reads
    coded_rows = flat[:hits.size * Bd].reshape(1, -1, Bd)        # the same bytes at the coded width
    w, gaps = 5, ("touch", "inside", "between", "past")
    for i, n in enumerate(lens):
        f = C.encode(rng.integers(0, 256, n).astype(np.uint8).tobytes(), h, kind)
        coded_rows[0, i, :len(f)] = np.frombuffer(f, np.uint8)
        if i == 7:
            coded_rows[0, i, h] ^= 1                             # an invalid row covers nothing
        hits["window"][0, i] = w
        plain, coded = C.frame_symbols(len(f), bits), X.coded_symbols(n, h, kind, bits)
        assert coded > plain + 1
        gap = gaps[i % 4]
        w += {"touch": L + coded, "inside": L + coded - 1, "between": L + plain + 1, "past": L + coded + 7}[gap] * Rn
    nw = len(lens)
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_hits, d_res = torch.from_numpy(hits.view(np.uint8).reshape(-1)).cuda(), \
        torch.from_numpy(results_bytes([nw]).reshape(-1)).cuda()
    d_rows = torch.from_numpy(flat).cuda()
    for coded in (True, False):
        view, width = (coded_rows, Bd) if coded else (rows, B)
        max_len = width - h - 2
        want, refs = coded_expected(hits, view, [nw], L, Rn, bits, h, kind, fec=X.CONV_K7 if coded else 0)
        o = dict(check=torch.full((hits.size * 16,), POISON, **u8), kept=torch.full((hits.size * 4,), POISON, **u8),
                 body=torch.full((hits.size * max_len,), POISON, **u8), summary=torch.full((32,), POISON, **u8))
        call = d.frames_check_coded_async if coded else d.frames_check_async
        call(d_hits, d_rows, d_res, 1, hits.shape[1], L, N, h, kind, o["check"], o["kept"].view(torch.int32),
             o["body"], o["summary"])
        torch.cuda.synchronize()
        shape = dict(check=(1, -1, 16), kept=(1, -1, 4), body=(1, -1, max_len), summary=(1, 32))
        same({k: v.cpu().numpy().reshape(shape[k]) for k, v in o.items()}, want, coded)
        if coded:
            cov = refs[0][0]["covered"].tolist()
            plain_cov = C.check_group(hits["window"][0, :nw], coded_rows[0, :nw], L, Rn, Z.span_of(bits, h, kind, 0),
                                      None, h, kind)[0]["covered"]
            assert sum(cov) >= 4 and sum(cov) > int(plain_cov.sum())       # the fixture's condition


# ---- end to end ------------------------------------------------------------------------------

E2E_L, E2E_LENS, E2E_HIT = 24, (5, 0, 12, 40, 9), (0, 2, 3)      # frames 0, 2 and 3 carry wrong tones


def e2e_stream(freqs, h=2, kind=C.CRC16, n=1024, hop=256, sigma=400.0, amplitude=8000.0, seed=91):
    """Five coded frames of different lengths as FSK with a random phase per
    symbol plus Gaussian noise, symbol boundaries on window starts; in three of
    them 3 well-separated payload symbols are sent on a wrong tone. Returns (x
    int16, word, N, the words' windows, datas, the sent payload rows)."""
    rng = np.random.default_rng(seed + len(freqs))
    K, Rn = len(freqs), n // hop
    bits = F.bits_per_symbol(K)
    word = rng.integers(0, K, E2E_L).astype(np.uint8)
    N = Z.symbols_for(max(E2E_LENS), bits, h, kind, X.CONV_K7) + 3
    datas = [rng.integers(0, 256, m).astype(np.uint8).tobytes() for m in E2E_LENS]
    seq, at, sent = [rng.integers(0, K, 9).astype(np.uint8)], [], []
    for f, data in enumerate(datas):
        at.append(sum(len(s) for s in seq))
        row = info_symbols(C.encode(data, h, kind), X.steps(len(data), h, kind), N, bits, rng, 0)
        sent.append(row.copy())
        if f in E2E_HIT:
            Sc = X.coded_symbols(len(data), h, kind, bits)
            for j in (Sc // 6, Sc // 2, (5 * Sc) // 6):
                row[j] = (row[j] + 1 + int(rng.integers(0, K - 1))) % K
        seq += [word, row, rng.integers(0, K, 8 + 3 * f).astype(np.uint8)]
    seq.append(rng.integers(0, K, 4).astype(np.uint8))
    truth = np.concatenate(seq)
    t = np.arange(n)
    ph = rng.uniform(0, 2 * np.pi, truth.size)
    w = 2 * np.pi * np.asarray(freqs, np.float64)[truth] / 48000.0
    v = amplitude * np.sin(w[:, None] * t[None, :] + ph[:, None]) + rng.normal(0.0, sigma, (truth.size, n))
    x = np.clip(np.round(v), -32768, 32767).astype(np.int16).reshape(-1)
    return np.ascontiguousarray(x), word, N, [a * Rn for a in at], datas, sent


@pytest.mark.parametrize("name", ["FSK2", "FSK8"])
def test_end_to_end(A, torch, name):
    """Detector, scan, decode and coded check in one call: all five bodies
    come back although the hard decisions of three rows differ from what was
    sent. The rows are the reference decode of the device's own powers. Then
    the same batch as two segments through demod_frames_segments_async +
    demod_frames_decode_async + demod_frames_check_coded_async."""
    freqs = getattr(F, name)
    h, kind = 2, C.CRC16
    K, bits, Rn = len(freqs), F.bits_per_symbol(len(freqs)), 4
    x, word, N, windows, datas, sent = e2e_stream(freqs)
    St, Bd, max_len = X.row_shape(N, bits, h, kind)
    u8 = dict(dtype=torch.uint8, device="cuda")
    with A.Demodulator(n=1024, hop=256, freqs=freqs) as d:
        W = (len(x) - 1024) // 256 + 1
        d_pcm = torch.from_numpy(x).cuda()
        d_sym, d_mag = torch.empty(W, **u8), torch.empty(W * K, dtype=torch.float32, device="cuda")
        d.batch_async(d_pcm, W, d_sym, d_mag)
        torch.cuda.synchronize()
        sym, P = d_sym.cpu().numpy(), d_mag.cpu().numpy().reshape(W, K)
        s_hits, payload, _, s_res = d.frames(x, word, max_errors=1, frame_symbols=N)
        nw = s_res["n_written"]
        assert s_res["phase"] == 0 and set(windows) <= set(s_hits["window"].tolist())
        for f, w0 in enumerate(windows):             # the hard decisions: wrong where a wrong tone was sent
            hard = payload[s_hits["window"].tolist().index(w0)]
            assert np.array_equal(hard, sym[w0 + (E2E_L + np.arange(N)) * Rn])
            Sc = X.coded_symbols(len(datas[f]), h, kind, bits)
            assert int((hard[:Sc] != sent[f][:Sc]).sum()) == (3 if f in E2E_HIT else 0), f
        h1 = np.zeros((1, nw), C.HIT_DTYPE)
        h1[0] = s_hits
        rows, dec, _ = reference(P, W, None, h1, [nw], E2E_L, Rn, N, h, kind)
        chk, kept, bodies, summ = C.check_group(s_hits["window"], rows[0], E2E_L, Rn,
                                                Z.span_of(bits, h, kind, X.CONV_K7), None, h, kind)
        assert bodies == datas and [int(s_hits["window"][i]) for i in kept] == windows
        for pcm in (x, d_pcm):
            hits, lengths, body, res, summary = d.frames_coded(pcm, word, max_errors=1, frame_symbols=N,
                                                              len_bytes=h, crc=kind)
            assert body == datas and lengths.tolist() == list(E2E_LENS)
            assert hits["window"].tolist() == windows and hits.tobytes() == s_hits[kept].tobytes()
            assert summary == dict(n_checked=nw, n_valid=int(summ["n_valid"]), n_kept=5, reserved=0)
            assert {f: res[f] for f in res if f != "metric"} == {f: s_res[f] for f in s_res if f != "metric"}
        # two segments, cut in the gap before frame 3
        cut = windows[3] - 4 * Rn
        first, count, cap = [0, cut], [cut, W - cut], 8
        seg = d.frames_segments(x, first, count, word, max_errors=1, frame_symbols=N, payload=False, packed=False)
        d_first = torch.from_numpy(np.array(first, np.int64)).cuda()
        d_count = torch.from_numpy(np.array(count, np.int32)).cuda()
        d_hits, d_results = torch.full((2 * cap * 16,), POISON, **u8), torch.empty(2 * RES_BYTES, **u8)
        d_work = torch.empty(A.frames_segments_workspace_size(d.cfg, 2, W), **u8)
        d_fwork = torch.full((A.frames_decode_workspace_size(d.cfg, 2, cap, N),), POISON, **u8)
        outs = dict(rows=torch.full((2 * cap * Bd,), POISON, **u8), decode=torch.full((2 * cap * 16,), POISON, **u8),
                    check=torch.full((2 * cap * 16,), POISON, **u8), kept=torch.full((2 * cap * 4,), POISON, **u8),
                    body=torch.full((2 * cap * max_len,), POISON, **u8), summary=torch.full((64,), POISON, **u8))
        d.frames_segments_async(d_sym, d_mag, W, d_first, d_count, 2, word, 1, N, d_hits, None, None, cap,
                                d_results, d_work)
        d.frames_decode_async(d_hits, d_mag, W, d_first, d_results, 2, cap, E2E_L, N, h, kind, outs["rows"],
                              outs["decode"], d_fwork)
        d.frames_check_coded_async(d_hits, outs["rows"], d_results, 2, cap, E2E_L, N, h, kind, outs["check"],
                                   outs["kept"].view(torch.int32), outs["body"], outs["summary"])
        torch.cuda.synchronize()
        h2 = d_hits.cpu().numpy().view(C.HIT_DTYPE).reshape(2, cap)
        n_written = [r[3]["n_written"] for r in seg]
        for s in range(2):                 # the device rows are the synchronous call's
            assert h2[s, :n_written[s]].tobytes() == seg[s][0].tobytes()
        rows2, dec2, _ = reference(P, W, first, h2, n_written, E2E_L, Rn, N, h, kind)
        want, refs = coded_expected(h2, rows2, n_written, E2E_L, Rn, bits, h, kind)
        want.update(rows=rows2, decode=dec2)
        shape = dict(rows=(2, cap, Bd), decode=(2, cap, 16), check=(2, cap, 16), kept=(2, cap, 4),
                     body=(2, cap, max_len), summary=(2, 32))
        same({k: v.cpu().numpy().reshape(shape[k]) for k, v in outs.items()}, want, "segments")
        assert [int(h2[s, i]["window"]) + first[s] for s in range(2) for i in refs[s][1]] == windows
        assert [b for s in range(2) for b in refs[s][2]] == datas
