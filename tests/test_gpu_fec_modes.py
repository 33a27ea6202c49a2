"""The coded modes on the GPU (include/demod.h "punctured and interleaved"):
frames_fec.hip's decode in every mode against the host decoder
demod_fec_frame_decode on the reference's soft values, byte for byte, over
poisoned buffers; guard bands around the powers; more rows than waves and
segments; capture and replay; the transmitter's ring symbols against the host
demod_tx_frame_symbols; Transmitter -> Receiver against tests/fec_modes_ref.py's
receiver on the device detector's own outputs, with and without a run of
zeroed samples; and the refusals of the device entries.

Kernel level as tests/test_gpu_frames_fec.py: test-made hits, results, tables
and powers on the device, so no detector and no scan run.
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
import rx_ref as RX
import tx_ref as T
from gpu_support import handle_fixture, phased, results_bytes, same as whole_same, torch  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPE_OF_R = {1: (1024, 1024), 4: (1024, 256)}       # (n, hop) of a handle with R phases
RES_BYTES = F.RESULT_DTYPE.itemsize
POISON = 0xFF
L0 = 8               # the word's symbols in the kernel-level tests (it is never read)
MAX_LEN = 40         # rows that hold every edge length of fec_modes_ref.edge_lengths


# handle(R, K): one Demodulator per (R, K), closed with the module.
handle = handle_fixture(lambda A, Rn, K: phased(A, SHAPE_OF_R, Rn, T.loop_tones(K)))


def air_symbols(air, N, bits, rng):
    """N row symbols: the air bits `air` (cut at the row's end), random bits behind them."""
    b = np.concatenate([air, rng.integers(0, 2, max(0, N * bits - air.size)).astype(np.uint8)])[:N * bits]
    return (b.reshape(N, bits) << np.arange(bits - 1, -1, -1, dtype=np.uint8)).sum(axis=1).astype(np.uint8)


def frame_row(rng, length, N, bits, h, kind, fec, flips=4):
    """A frame of `length` random data bytes in the mode's air order with
    `flips` inverted air bits, as N row symbols; and its checked frame."""
    frame = C.encode(rng.integers(0, 256, length).astype(np.uint8).tobytes(), h, kind)
    air = Z.encode_air(frame, X.steps(length, h, kind), fec)
    if flips:
        air[rng.choice(min(air.size, N * bits), flips, replace=False)] ^= 1
    return air_symbols(air, N, bits, rng), frame


def powers_for(sym, K, rng):
    """P float32 [W][K]: the symbol's tone 1000 .. 1999, the others 1 .. 299."""
    P = rng.integers(1, 300, (sym.size, K)).astype(np.float32)
    P[np.arange(sym.size), sym] = rng.integers(1000, 2000, sym.size)
    return P


def lay_rows(rows_sym, K, Rn, rng, L=L0, lead=3, tail=5):
    """The rows' symbols one behind the other on phase `lead` % R, symbol j of
    row r at window start_r + (L + j) R; random symbols everywhere else.
    Returns (P [W][K], start windows)."""
    N = len(rows_sym[0])
    span = (L + N) * Rn
    W = lead + len(rows_sym) * span + tail
    sym = rng.integers(0, K, W).astype(np.uint8)
    starts = []
    for r, row in enumerate(rows_sym):
        s = lead + r * span
        sym[s + L * Rn:s + (L + N) * Rn:Rn] = row
        starts.append(s)
    return powers_for(sym, K, rng), np.array(starts, np.uint64)


def reference(A, P, n_windows, first, hits, n_written, L, Rn, N, h, kind, fec, poison=POISON):
    """rows [G][max_frames][Bd] and decode [G][max_frames][16] whole: the host
    decoder demod_fec_frame_decode on the reference's soft values of each row,
    laid over poison. Rows with the same absolute start decode once. Also {key:
    (bytes written, record)}."""
    n_groups, max_frames = hits.shape
    bits = F.bits_per_symbol(P.shape[1])
    St, Bd, max_len = Z.row_shape(N, bits, h, kind, fec)
    rows = np.full((n_groups, max_frames, Bd), poison, np.uint8)
    dec = np.full((n_groups, max_frames, 16), poison, np.uint8)
    soft = X.soft_bits(P[:n_windows])
    done = {}
    for g in range(n_groups):
        base = 0 if first is None else min(int(first[g]), n_windows)
        for i in range(min(int(n_written[g]), max_frames)):
            w = int(hits["window"][g, i])
            key = (base, w) if w < n_windows else None
            if key not in done:
                q = X.row_soft(soft, n_windows, base, w, L, Rn, N)
                written, rec = A.fec_frame_decode(q, h, kind, fec)
                done[key] = (written, np.array([tuple(rec[f] for f in X.DECODE_DTYPE.names)], X.DECODE_DTYPE))
            written, rec = done[key]
            rows[g, i, :len(written)] = np.frombuffer(written, np.uint8)
            dec[g, i] = rec.view(np.uint8)
    return rows, dec, done


class Run:
    """One decode call on test-made inputs; rows, decode and a workspace of
    exactly the mode's size poisoned."""

    def __init__(self, A, torch, P, hits, n_written, first=None, n_windows=None, poison=POISON, work_poison=None,
                 d_mag=None):
        self.A, self.torch = A, torch
        self.n_groups, self.max_frames = hits.shape
        self.W = P.shape[0] if n_windows is None else n_windows
        self.inputs = [np.ascontiguousarray(hits).view(np.uint8).reshape(-1),
                       np.ascontiguousarray(P, np.float32).reshape(-1), results_bytes(n_written).reshape(-1)]
        if first is not None:
            self.inputs.append(np.array([int(f) for f in first], "<u8").view(np.int64))
        self.d_in = [torch.from_numpy(a.copy()).cuda() for a in self.inputs]
        if d_mag is not None:
            self.d_in[1] = d_mag
        self.poison = poison
        self.work_poison = poison if work_poison is None else work_poison

    def __call__(self, d, L, N, h, kind, fec, stream=0):
        torch = self.torch
        rows = self.n_groups * self.max_frames
        Bd = Z.row_shape(N, F.bits_per_symbol(d.k), h, kind, fec)[1]
        u8 = dict(dtype=torch.uint8, device="cuda")
        self.d_rows, self.d_dec = torch.full((rows * Bd,), self.poison, **u8), torch.full((rows * 16,), self.poison, **u8)
        need = self.A.fec_decode_workspace_size(d.cfg, self.n_groups, self.max_frames, N, fec)
        self.d_work = torch.full((need,), self.work_poison, **u8)
        d.frames_decode_async(self.d_in[0], self.d_in[1], self.W, self.d_in[3] if len(self.d_in) > 3 else None,
                              self.d_in[2], self.n_groups, self.max_frames, L, N, h, kind, self.d_rows, self.d_dec,
                              self.d_work, fec=fec, stream=stream)
        return self.results(Bd)

    def results(self, Bd):
        self.torch.cuda.synchronize()
        for t, a in zip(self.d_in, self.inputs):
            assert t.cpu().numpy().tobytes() == a.tobytes(), "an input was written to"     # NaNs compare as bytes
        return (self.d_rows.cpu().numpy().reshape(self.n_groups, self.max_frames, Bd),
                self.d_dec.cpu().numpy().reshape(self.n_groups, self.max_frames, 16))


same = functools.partial(whole_same, names=("rows", "decode"))


def one_group(starts, max_frames=None):
    hits = np.zeros((1, max_frames or len(starts)), C.HIT_DTYPE)
    hits["window"][0, :len(starts)] = starts
    return hits


def shape_rows(rng, N, bits, h, kind, fec):
    """The rows of one shape: the edge lengths with 4 inverted air bits each and
    a header of max_len + 1. Returns (rows, the checked frames)."""
    St, Bd, max_len = Z.row_shape(N, bits, h, kind, fec)
    rows, frames = [], []
    for n in Z.edge_lengths(max_len, h, kind, fec):
        row, frame = frame_row(rng, n, N, bits, h, kind, fec)
        rows.append(row)
        frames.append(frame)
    info = (max_len + 1).to_bytes(h, "big") + rng.integers(0, 256, Bd).astype(np.uint8).tobytes()
    rows.append(air_symbols(Z.encode_air(info, St, fec), N, bits, rng))
    return rows, frames


# ---- 8. decode parity ---------------------------------------------------------------------

@pytest.mark.parametrize("h", [1, 2])
@pytest.mark.parametrize("Rn", [1, 4])
@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("fec", Z.MODES)
def test_decode_parity(A, torch, handle, fec, K, Rn, h):
    """Every mode (0x01 the control) at K 2 and 8 (at 3 bits a symbol the
    blocks straddle symbols), R 1 and 4, h 1 and 2, both CRCs at K 2: the edge
    lengths with 4 inverted air bits each, a header of max_len + 1, and a hit
    whose tail lies past n_windows (erasures). d_rows and d_decode whole equal
    demod_fec_frame_decode's bytes over the same poison; d_work is exactly the
    mode's size."""
    d = handle(Rn, K)
    bits = F.bits_per_symbol(K)
    statuses, clean = set(), 0
    for kind in ((C.CRC16, C.CRC32) if K == 2 else (C.CRC16 if h == 1 else C.CRC32,)):
        N = Z.symbols_for(MAX_LEN, bits, h, kind, fec) + 1
        rng = np.random.default_rng(fec * 1000 + K * 10 + h + kind)
        rows, frames = shape_rows(rng, N, bits, h, kind, fec)
        P, starts = lay_rows(rows, K, Rn, rng)
        W = len(P)
        late = [W - (L0 + (3 * N) // 4) * Rn, W - (L0 + 300 // bits) * Rn, W - 1]     # the tail past n_windows
        all_starts = np.concatenate([starts, np.array(late, np.uint64)])
        hits = one_group(all_starts, len(all_starts) + 2)
        want = reference(A, P, W, None, hits, [len(all_starts)], L0, Rn, N, h, kind, fec)
        got = Run(A, torch, P, hits, [len(all_starts)])(d, L0, N, h, kind, fec)
        same(got, want[:2], (hex(fec), K, Rn, h, kind))
        for i, frame in enumerate(frames):
            written, rec = want[2][0, int(starts[i])]
            clean += written == frame and rec["status"][0] == X.OK
        statuses |= {int(v[1]["status"][0]) for v in want[2].values()}
    assert statuses == {X.OK, X.BAD_LENGTH} and clean >= 2


# ---- 9. guards -----------------------------------------------------------------------------

@pytest.mark.parametrize("fec,K,Rn", [(0x41, 2, 4), (0x51, 8, 1), (0x61, 8, 4), (0x21, 2, 1)])
def test_guards(A, torch, handle, fec, K, Rn):
    """d_mags holds exactly n_windows K floats between guard bands: NaN, then
    loud finite powers (a NaN read would pass for an erasure; a loud one
    cannot). Rows whose interleaved block reaches past the end decode to the
    reference's bytes under both, so the guards are not read. d_work is exactly
    the mode's size and poisoned on entry."""
    d = handle(Rn, K)
    bits, h, kind = F.bits_per_symbol(K), 1, C.CRC16
    N = Z.symbols_for(MAX_LEN, bits, h, kind, fec) + 1
    rng = np.random.default_rng(fec + K)
    rows, _ = shape_rows(rng, N, bits, h, kind, fec)
    P, starts = lay_rows(rows, K, Rn, rng, tail=0)
    W = len(P)
    late = [W - (L0 + j) * Rn - 1 for j in (0, 1, 255 // bits, 256 // bits, 257 // bits, N // 2, N - 2)]
    all_starts = np.concatenate([starts, np.array(late + [W - 1, W, W + 1], np.uint64)])
    hits = one_group(all_starts)
    want = reference(A, P, W, None, hits, [len(all_starts)], L0, Rn, N, h, kind, fec)
    for guard in ("nan", "loud"):
        if guard == "nan":
            body, chk = G.guarded(torch, W * K, torch.float32, G.F32_GUARD, G.F32_GUARD, G.F32_POISON)
        else:
            loud = rng.integers(1, 3, G.F32_GUARD + W * K + G.F32_GUARD).astype(np.float32) * np.float32(1.0e6)
            body = torch.from_numpy(loud).cuda()[G.F32_GUARD:G.F32_GUARD + W * K]
        body.copy_(torch.from_numpy(P.reshape(-1)))
        for work_poison in (0xFF, 0x00):
            run = Run(A, torch, P, hits, [len(all_starts)], d_mag=body, work_poison=work_poison)
            got = run(d, L0, N, h, kind, fec)
            same(got, want[:2], (hex(fec), guard, work_poison))
            assert run.d_work.numel() == A.fec_decode_workspace_size(d.cfg, 1, len(all_starts), N, fec)
        if guard == "nan":
            chk(written=False)
    metric = want[1].view(X.DECODE_DTYPE)["metric"]
    assert np.isfinite(metric.astype(np.float64)).all() and (np.abs(metric.astype(np.int64)) < 2 ** 28).all()


# ---- 10. more rows than waves, segments ---------------------------------------------------------

def pool(rng, K, Rn, h, kind, fec, N, count):
    """`count` rows of one shape (frames of drawn lengths, every fourth a
    random row) laid in one batch: (P, starts)."""
    bits = F.bits_per_symbol(K)
    max_len = Z.row_shape(N, bits, h, kind, fec)[2]
    rows = [rng.integers(0, K, N).astype(np.uint8) if r % 4 == 3 else
            frame_row(rng, int(rng.integers(0, max_len + 1)), N, bits, h, kind, fec)[0] for r in range(count)]
    return lay_rows(rows, K, Rn, rng)


def test_more_rows_than_waves(A, torch, handle):
    """Mode 0x51, 1024 groups x 32 minimal rows (one block): 16 waves a group,
    each takes two rows and reuses its workspace slot; two workspace poisons."""
    fec, K, Rn, h, kind = 0x51, 2, 1, 1, C.CRC16
    d = handle(Rn, K)
    N = Z.BLOCK
    assert Z.row_shape(N, 1, h, kind, fec) is not None and Z.row_shape(N - 1, 1, h, kind, fec) is None
    rng = np.random.default_rng(1024)
    P, starts = pool(rng, K, Rn, h, kind, fec, N, 48)
    hits = np.zeros((1024, 32), C.HIT_DTYPE)
    hits["window"] = starts[rng.integers(0, len(starts), hits.shape)]
    counts = rng.integers(0, 33, 1024).tolist()
    counts[0], counts[1], counts[-1] = 32, 0, 32
    want = reference(A, P, len(P), None, hits, counts, L0, Rn, N, h, kind, fec)
    for work_poison in (0xFF, 0x00):
        same(Run(A, torch, P, hits, counts, work_poison=work_poison)(d, L0, N, h, kind, fec), want[:2], work_poison)


def test_segments(A, torch, handle):
    """Mode 0x51 with a segment table: the same rows under two different
    first[] give identical bytes, and a first[] above n_windows is clamped
    (every value an erasure)."""
    fec, K, Rn, h, kind = 0x51, 8, 4, 2, C.CRC16
    d = handle(Rn, K)
    N = Z.symbols_for(6, 3, h, kind, fec) + 2
    rng = np.random.default_rng(8)
    P, starts = pool(rng, K, Rn, h, kind, fec, N, 8)
    W = len(P)
    shift = 3 * (L0 + N) * Rn
    both = np.concatenate([P, P[shift:], P[:shift]])             # the same rows again, `shift` windows earlier
    rel = starts[3:7] - np.uint64(shift)
    hits = np.zeros((4, 5), C.HIT_DTYPE)
    hits["window"][0, :4], hits["window"][1, :4] = rel, starts[:4]
    hits["window"][2, :4], hits["window"][3, :4] = rel, starts[:4]
    first, counts = [shift, 0, W, 2 ** 64 - 1], [4, 4, 4, 3]
    want = reference(A, both, 2 * W, first, hits, counts, L0, Rn, N, h, kind, fec)
    got = Run(A, torch, both, hits, counts, first=first)(d, L0, N, h, kind, fec)
    same(got, want[:2])
    for a in got:
        assert np.array_equal(a[0], a[2])                        # another first[], another slot
    zero = A.fec_frame_decode(np.zeros(N * 3, np.int8), h, kind, fec)
    assert bytes(got[0][3, 0, :len(zero[0])]) == zero[0] and got[1][3, 0].view(X.DECODE_DTYPE)[0]["metric"] == 0


# ---- 11. capture and replay -----------------------------------------------------------------------

def test_capture_and_replay(A, torch, handle):
    """The decode in mode 0x51 in a graph on a side stream, replayed after the
    powers were rewritten in place and the outputs and the workspace poisoned
    again: each replay's bytes are the reference's for that content."""
    fec, K, Rn, h, kind = 0x51, 8, 4, 1, C.CRC16
    d = handle(Rn, K)
    bits = 3
    N = Z.symbols_for(MAX_LEN, bits, h, kind, fec) + 1
    contents = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        rows, _ = shape_rows(rng, N, bits, h, kind, fec)
        contents.append(lay_rows(rows, K, Rn, rng))
    starts = contents[0][1]
    assert np.array_equal(starts, contents[1][1]) and not np.array_equal(contents[0][0], contents[1][0])
    hits = one_group(starts, len(starts) + 1)
    wants = {po: [reference(A, P, len(P), None, hits, [len(starts)], L0, Rn, N, h, kind, fec, po) for P, _ in contents]
             for po in (POISON, 0x5A)}
    assert not np.array_equal(wants[POISON][0][0], wants[POISON][1][0])
    run = Run(A, torch, contents[0][0], hits, [len(starts)])
    Bd = Z.row_shape(N, bits, h, kind, fec)[1]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = run(d, L0, N, h, kind, fec, stream=side.cuda_stream)        # an eager call of the shape first
    same(got, wants[POISON][0][:2], "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        d.frames_decode_async(run.d_in[0], run.d_in[1], run.W, None, run.d_in[2], 1, hits.shape[1], L0, N, h, kind,
                              run.d_rows, run.d_dec, run.d_work, fec=fec,
                              stream=torch.cuda.current_stream().cuda_stream)
    for po in (POISON, 0x5A):
        for (P, _), want in zip(contents, wants[po]):
            run.inputs[1] = np.ascontiguousarray(P, np.float32).reshape(-1)
            run.d_in[1].copy_(torch.from_numpy(run.inputs[1]))
            for t in (run.d_rows, run.d_dec, run.d_work):
                t.fill_(po)
            torch.cuda.synchronize()
            g.replay()
            same(run.results(Bd), want[:2], ("replay", po))


# ---- 12. transmitter ---------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("fec", Z.MODES)
def test_transmitter_symbols(A, torch, fec, K):
    """demod_tx_encode_async's ring symbols equal the host
    demod_tx_frame_symbols in every mode: lengths 0, the lengths nearest a
    block edge and max_len, two streams, gap 0 and poison behind the frames."""
    n, S, h, kind = 256, 2, 1, C.CRC16
    bits = F.bits_per_symbol(K)
    lens = Z.edge_lengths(MAX_LEN, h, kind, fec)
    word = (np.arange(11) * 5) % K
    rng = np.random.default_rng(fec + K)
    datas = [rng.integers(0, 256, ln).astype(np.uint8).tobytes() for ln in lens]
    counts = [11 + Z.span(ln, bits, h, kind, fec) for ln in lens]
    ring = sum(counts) + 9
    x = A.make_tx_cfg(word, h, kind, fec, MAX_LEN, 0, (0,), 8000, 0, 0, ring, len(lens), 2880)
    want = [A.tx_frame_symbols(x, K, data) for data in datas]
    assert [len(w) for w in want] == counts
    records = np.zeros((S, len(lens)), T.RECORD_DTYPE)
    blob, at = b"", []
    for data in datas:
        at.append(len(blob))
        blob += data
    for s in range(S):
        order = range(len(lens)) if s == 0 else range(len(lens) - 1, -1, -1)
        for i, f in enumerate(order):
            records[s, i] = (lens[f], at[f])
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_state = torch.zeros(S * 40, **u8)
    d_ring = torch.full((S * ring,), POISON, **u8)
    d_place = torch.full((S * len(lens) * 16,), POISON, **u8)
    d_rec = torch.from_numpy(records.view(np.uint8).reshape(-1).copy()).cuda()
    d_count = torch.from_numpy(np.full(S, len(lens), np.uint32).view(np.int32)).cuda()
    d_bytes = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    with A.Demodulator(n=n, hop=n // 4, freqs=T.loop_tones(K)) as d:
        d.tx_encode_async(x, d_state, d_ring, d_rec, d_count, d_bytes, len(blob), S, d_place)
        torch.cuda.synchronize()
    place = d_place.cpu().numpy().view(T.PLACE_DTYPE).reshape(S, len(lens))
    got = d_ring.cpu().numpy().reshape(S, ring)
    assert (place["status"] == T.OK).all()
    for s in range(S):
        order = list(range(len(lens))) if s == 0 else list(range(len(lens) - 1, -1, -1))
        for i, f in enumerate(order):
            start, cnt = int(place["start"][s, i]), int(place["symbols"][s, i])
            assert cnt == counts[f] and start == sum(counts[g] for g in order[:i])
            bad = np.flatnonzero(got[s, start:start + cnt] != want[f])
            assert bad.size == 0, (hex(fec), K, s, lens[f], bad[:6].tolist())
        assert (got[s, sum(counts):] == POISON).all()


# ---- 13. link -----------------------------------------------------------------------------------------

LINK_N, LINK_HOP, LINK_K, LINK_S, LINK_L, LINK_H, LINK_KIND = 1024, 256, 2, 3, 16, 1, C.CRC16
LINK_LENS = (0, 24, 7)
LINK_PACKET = 48000                  # a second of audio a push: a frame spans several pushes
LINK_DROPS = (0, 100, 200)           # samples cut from the head of each stream: three window offsets
LINK_SHAPE = (LINK_K, LINK_H, LINK_KIND)
LINK_SHAPE_8 = (8, 2, C.CRC32)       # 3 bits a symbol: a 256-bit block ends inside a symbol


def link_run(A, torch, fec, zero=None, shape=LINK_SHAPE):
    """Transmitter -> (samples on the host, `zero` = (frame, first payload
    symbol, symbols) zeroed in every stream) -> Receiver, in LINK_PACKET pushes.
    shape: (K, h, CRC). Returns (datas, per stream (pushed samples, sizes),
    pushes: (records, bodies), N, ring, the word)."""
    K, h, kind = shape
    bits = F.bits_per_symbol(K)
    rng = np.random.default_rng(4100 + fec)
    word = rng.integers(0, K, LINK_L).astype(np.uint8)
    datas = [rng.integers(0, 256, ln).astype(np.uint8).tobytes() for ln in LINK_LENS]
    max_len, gap = max(LINK_LENS), 3
    per = [LINK_L + Z.span(len(dd), bits, h, kind, fec) + gap for dd in datas]
    N = Z.symbols_for(max_len, bits, h, kind, fec)
    symbols = 3 + sum(per) + N + 8
    total = -(-symbols * LINK_N // LINK_PACKET) * LINK_PACKET
    ring = total // LINK_HOP + 64
    x = A.make_tx_cfg(word, h, kind, fec, max_len, gap, (0, 1), 8000, 400, 77, sum(per) + 5, len(datas),
                      LINK_PACKET)
    freqs = T.loop_tones(K)
    pcm = [[] for _ in range(LINK_S)]
    with A.Transmitter(LINK_S, x, n=LINK_N, hop=LINK_HOP, freqs=freqs) as tx:
        for at in range(0, total, LINK_PACKET):
            if at == LINK_PACKET:
                accepted, place = tx.send([(s, dd) for s in range(LINK_S) for dd in datas])
                assert accepted == LINK_S * len(datas) and (place["status"] == T.OK).all()
            out = tx.pull(LINK_PACKET)
            for s in range(LINK_S):
                pcm[s].append(out[s])
    pcm = [np.concatenate(p) for p in pcm]
    if zero is not None:
        f, j, cnt = zero
        a = (int(place["start"][f]) + LINK_L + j) * LINK_N
        for s in range(LINK_S):
            pcm[s][a:a + cnt * LINK_N] = 0
    pcm = [p[drop:] for p, drop in zip(pcm, LINK_DROPS)]
    rxcfg = A.make_rx_cfg(word, 2, N, h, kind, fec, 8, ring)
    pushes, sizes = [], [[] for _ in range(LINK_S)]
    with A.Receiver(LINK_S, rxcfg, n=LINK_N, hop=LINK_HOP, freqs=freqs) as rx:
        for at in range(0, total, LINK_PACKET):
            packets = [p[at:at + LINK_PACKET] for p in pcm]
            for s in range(LINK_S):
                sizes[s].append(len(packets[s]))
            fr, bodies, summ = rx.push([p if len(p) else None for p in packets])
            assert summ["n_frames"] == len(fr)
            pushes.append((fr, bodies))
    return datas, list(zip(pcm, sizes)), pushes, N, ring, word


def link_reference(A, fec, streams, N, ring, word, shape=LINK_SHAPE):
    """fec_modes_ref.receiver on the device detector's own outputs, push by push."""
    import link_ref as LR
    K, h, kind = shape
    R = LINK_N // LINK_HOP
    cuts = []
    with A.Demodulator(n=LINK_N, hop=LINK_HOP, freqs=T.loop_tones(K)) as d:
        for pcm, sizes in streams:
            W = (len(pcm) - LINK_N) // LINK_HOP + 1
            sym, P = d.batch(pcm[:(W - 1) * LINK_HOP + LINK_N], mags=True)
            cuts.append(LR.pieces(sym, P, sizes, LINK_N, LINK_HOP))
    ref = RX.Rx(LINK_S, K, R, word, 2, N, h, kind, fec, 8, ring)
    return [ref.push([cuts[s][i] for s in range(LINK_S)]) for i in range(len(cuts[0]))]


def delivered(pushes, s):
    return [b for fr, bodies in pushes for f, b in zip(fr, bodies) if int(f["stream"]) == s]


def link_holds(A, torch, fec, shape):
    datas, streams, pushes, N, ring, word = link_run(A, torch, fec, shape=shape)
    want = link_reference(A, fec, streams, N, ring, word, shape)
    for i, ((fr, bodies), (w_fr, w_bodies, _)) in enumerate(zip(pushes, want)):
        assert fr.tobytes() == w_fr.tobytes() and bodies == w_bodies, ("push", i, fr, w_fr)
    for s in range(LINK_S):
        assert delivered(pushes, s) == datas, (hex(fec), s)


@pytest.mark.parametrize("fec", [0x11, 0x41, 0x61, 0x21, 0x51])
def test_link(A, torch, fec):
    """Transmitter -> Receiver, 3 streams at three sample offsets, in every
    mapped mode: every push equals the host reference on the same detector
    outputs, and every frame of every stream comes back."""
    link_holds(A, torch, fec, LINK_SHAPE)


def test_link_8_tones(A, torch):
    """The same in mode 0x51 at 8 tones, h 2, CRC-32: punctured and
    interleaved, the 256-bit blocks ending inside a symbol."""
    link_holds(A, torch, 0x51, LINK_SHAPE_8)


@pytest.mark.parametrize("fec", [0x41, 0x01])
def test_link_with_dropout(A, torch, fec):
    """The same with the samples of 12 consecutive payload symbols of frame 1
    zeroed: every push equals the host reference on the same detector outputs;
    the interleaved mode keeps the frame."""
    datas, streams, pushes, N, ring, word = link_run(A, torch, fec, zero=(1, 40, 12))
    for i, ((fr, bodies), (w_fr, w_bodies, _)) in enumerate(zip(pushes, link_reference(A, fec, streams, N, ring, word))):
        assert fr.tobytes() == w_fr.tobytes() and bodies == w_bodies, ("push", i, fr, w_fr)
    if fec & Z.INTERLEAVE:
        for s in range(LINK_S):
            assert delivered(pushes, s) == datas, (hex(fec), s)


# ---- 14. refusals -----------------------------------------------------------------------------------------

def test_refusals(A, torch, handle):
    """fec of 2, 0x10, 0x31 and 0x81 at every device entry that takes it, 0x41
    with K = 3, an interleaved row shorter than one block, and work_bytes one
    below the mode's size: DEMOD_BAD_ARG before any launch, the outputs stay
    poison. The same calls, legal, run."""
    lib = A.load_library()
    d = handle(4, 2)
    S, cap, N, L, W = 3, 16, 600, 8, 5000
    rows = S * cap
    u8 = dict(dtype=torch.uint8, device="cuda")

    def poison(nbytes):
        return torch.full((nbytes,), 0xFF, **u8)
    d_hits, d_res = torch.zeros(rows * 16, **u8), torch.zeros(S * RES_BYTES, **u8)
    d_mag = torch.ones(W * 2, dtype=torch.float32, device="cuda")
    d_state = torch.zeros(S * 40, **u8)
    Bd = max(Z.row_shape(N, 1, 1, C.CRC16, f)[1] for f in Z.MODES)
    need = {f: A.fec_decode_workspace_size(d.cfg, S, cap, N, f) for f in Z.MODES}
    assert need[0x21] > need[0x11] > need[0x01] == A.frames_decode_workspace_size(d.cfg, S, cap, N)
    assert need[0x41] == S * cap * 256 * 8
    d_rows, d_dec, d_work = poison(rows * Bd), poison(rows * 16), poison(max(need.values()))
    d_check, d_kept, d_body, d_sum = poison(rows * 16), poison(rows * 4), poison(rows * Bd), poison(S * 32)
    d_frames, d_bodies, d_rsum = poison(rows * 32), poison(rows * Bd), poison(32)
    d_cwork = poison(A.rx_collect_workspace_size(d.cfg, S))
    ph, pm, pr, po, pd, pw = (t.data_ptr() for t in (d_hits, d_mag, d_res, d_rows, d_dec, d_work))
    pc, pk, pb, ps = (t.data_ptr() for t in (d_check, d_kept, d_body, d_sum))
    kind = A.DEMOD_CRC16_CCITT_FALSE

    def decode(fec, h=d._h, n=N, work_bytes=None):
        return lib.demod_frames_decode_async(h, ph, pm, W, None, pr, S, cap, L, n, 1, kind, fec, po, pd, pw,
                                             d_work.numel() if work_bytes is None else work_bytes, None)

    def check(fec, h=d._h, n=N):
        return lib.demod_frames_check_coded_async(h, ph, po, pr, S, cap, L, n, 1, kind, fec, pc, pk, pb, ps, None)

    def collect(fec, h=d._h, n=N):
        return lib.demod_rx_collect_async(h, d_state.data_ptr(), ph, pr, pc, pk, pb, ps, S, cap, L, n, 1, kind, fec,
                                          d_frames.data_ptr(), d_bodies.data_ptr(), d_rsum.data_ptr(),
                                          d_cwork.data_ptr(), d_cwork.numel(), None)
    for fec in Z.BAD_MODES:
        assert decode(fec) == A.DEMOD_BAD_ARG and check(fec) == A.DEMOD_BAD_ARG and collect(fec) == A.DEMOD_BAD_ARG, fec
    assert decode(0) == A.DEMOD_BAD_ARG and check(0) == A.DEMOD_BAD_ARG
    for fec in Z.MODES:
        assert decode(fec, work_bytes=need[fec] - 1) == A.DEMOD_BAD_ARG, fec
        with pytest.raises(A.DemodError):
            d.frames_decode_async(d_hits, d_mag, W, None, d_res, S, cap, L, N, 1, kind, d_rows, d_dec,
                                  d_work[:need[fec] - 1], fec=fec)
    for fec in (0x41, 0x51, 0x61):                       # shorter than one block
        assert decode(fec, n=255) == A.DEMOD_BAD_ARG and check(fec, n=255) == A.DEMOD_BAD_ARG
        assert collect(fec, n=255) == A.DEMOD_BAD_ARG
    with A.Demodulator(n=1024, hop=256, freqs=(1500.0, 2250.0, 3000.0)) as k3:
        assert decode(0x41, h=k3._h) == A.DEMOD_BAD_ARG and check(0x41, h=k3._h) == A.DEMOD_BAD_ARG
        assert collect(0x41, h=k3._h) == A.DEMOD_BAD_ARG
        assert lib.demod_fec_decode_workspace_size(ctypes.byref(k3.cfg), S, cap, N, 0x41) == 0
        with pytest.raises(A.DemodError):
            k3.frames_coded(np.zeros(8192, np.int16), [0, 1], frame_symbols=N, fec=0x41)
    with pytest.raises(A.DemodError):
        d.frames_coded(np.zeros(8192, np.int16), [0, 1], frame_symbols=N, fec=0x31)
    torch.cuda.synchronize()
    for t in (d_rows, d_dec, d_work, d_check, d_kept, d_body, d_sum, d_frames, d_bodies, d_rsum, d_cwork):
        assert bool((t == 0xFF).all()), "a refused call wrote"
    # and the same calls, legal, run: three empty groups
    for fec in Z.MODES:
        assert decode(fec, work_bytes=need[fec]) == A.DEMOD_OK and check(fec) == A.DEMOD_OK, fec
    torch.cuda.synchronize()
    assert not d_sum.cpu().numpy().any()
    for t in (d_rows, d_dec, d_work, d_check, d_kept, d_body):
        assert bool((t == 0xFF).all())
