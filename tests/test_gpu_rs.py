"""The Reed-Solomon outer code on the GPU (include/demod.h "Reed-Solomon
outer code"): frames_rs.hip's stage on rows uploaded from the host against the
host decoder demod_rs_frame_decode, byte for byte, rows and records, between
guard bands and over poison; more rows than waves; the stage captured behind
the scan and replayed; the refusals of the device entries; demod_frames_coded
and demod_rx_push in a plain and a coded parity mode against the host chain
(tests/rs_chain_ref.py); and the transmitter's symbols against
demod_tx_frame_symbols, with a loop into the receiver.
"""
import ctypes
import functools

import numpy as np
import pytest

import fec_modes_ref as Z
import frames_check_ref as C
import frames_ref as F
import guards as G
import rs_cases as TC
import rs_chain_ref as H
import rs_ref as R
import tx_ref as T
from gpu_support import handle_fixture, results_bytes, same as whole_same, torch  # noqa: F401

pytestmark = pytest.mark.gpu

RES_BYTES = F.RESULT_DTYPE.itemsize
GUARD = 4096
POISON = 0xFF


# handle(K): one Demodulator (n 1024, hop 256) per K, closed with the module.
handle = handle_fixture(lambda A, K: A.Demodulator(n=1024, hop=256, freqs=T.loop_tones(K)))


def host_stage(A, rows, counts, max_frames, h, kind, fec):
    """demod_rs_frame_decode over rows i < min(count_g, max_frames) of every
    group; the other rows stay, their records stay POISON."""
    n_groups = len(counts)
    out = rows.copy().reshape(n_groups, max_frames, -1)
    rec = np.full((n_groups, max_frames, 16), POISON, np.uint8)
    memo = {}
    for g in range(n_groups):
        for i in range(min(int(counts[g]), max_frames)):
            key = out[g, i].tobytes()
            if key not in memo:
                got, r, _ = A.rs_frame_decode(out[g, i], h, kind, fec)
                memo[key] = (got, np.array([tuple(r[f] for f in A.FRAME_RS_DTYPE.names)], A.FRAME_RS_DTYPE))
            out[g, i] = memo[key][0]
            rec[g, i] = memo[key][1].view(np.uint8)
    return out, rec


def run_stage(A, torch, d, rows, counts, max_frames, N, h, kind, fec, stream=0):
    """The stage on rows [n_groups * max_frames][W] between guard bands:
    (rows, records [..][16]) after it, the guards checked."""
    n_groups, W = len(counts), rows.shape[-1]
    d_rows, chk_rows = G.guarded(torch, n_groups * max_frames * W, torch.uint8, GUARD, GUARD, POISON)
    d_rs, chk_rs = G.guarded(torch, n_groups * max_frames * 16, torch.uint8, GUARD, GUARD, POISON)
    d_rows.copy_(torch.from_numpy(np.ascontiguousarray(rows).reshape(-1)))
    res = results_bytes(counts).reshape(-1)
    d_res = torch.from_numpy(res.copy()).cuda()
    d.frames_rs_async(d_rows, d_res, n_groups, max_frames, N, h, kind, fec, d_rs, stream=stream)
    chk_rows(written=False)
    chk_rs(written=False)
    assert d_res.cpu().numpy().tobytes() == res.tobytes(), "the results were written to"
    return (d_rows.cpu().numpy().reshape(n_groups, max_frames, W), d_rs.cpu().numpy().reshape(n_groups, max_frames, 16))


same = functools.partial(whole_same, names=("rows", "records"))


def case_rows(A, flag, h, kind, W, rng, lengths=None, patterns=TC.PATTERNS):
    """The CPU test's cases as rows of W bytes: every edge length that fits,
    every error pattern; random bytes behind each frame. Then a header of
    max_len + 1 (where h bytes can say it) and two random rows."""
    P, c = R.PARITY[flag], C.CRC_BYTES[kind]
    rows = []
    for length in (TC.edge_lengths(h, c, P) if lengths is None else lengths):
        if R.frame_size(h + length + c, P) > W:
            continue
        data = bytes(rng.integers(0, 256, length, dtype=np.uint8))
        sent = A.rs_frame_encode(data, h, kind, flag)
        for pattern in patterns:
            row = bytearray(sent + bytes(rng.integers(0, 256, W - len(sent), dtype=np.uint8)))
            TC.corrupt(row, h + length + c, P, h, pattern, rng)
            rows.append(np.frombuffer(bytes(row), np.uint8))
    most = R.max_len(W, h, c, P)
    if most + 1 < 256 ** h:   # else the header cannot name a length the row does not hold
        rows.append(np.frombuffer((most + 1).to_bytes(h, "big") + bytes(rng.integers(0, 256, W - h, dtype=np.uint8)),
                                  np.uint8))
    return rows + [rng.integers(0, 256, W).astype(np.uint8) for _ in range(2)]


# ---- 1. the stage against the host decoder ---------------------------------------------------

@pytest.mark.parametrize("conv", [0, 1])
@pytest.mark.parametrize("h", [1, 2])
@pytest.mark.parametrize("flag", TC.FLAGS)
def test_stage_against_host(A, torch, handle, flag, h, conv):
    """Rows of 320 bytes (h 1) or 800 (h 2: three codewords): every length and
    pattern of tests/test_rs_cpu.py under both CRC kinds as one group, with two
    rows past the count; then three groups with counts 0, 2 and max_frames + 5.
    conv 1: the same rows as the decoded rows of mode 0x01, whose width is Bd."""
    d = handle(2)
    W = 320 if h == 1 else 800
    N = 2 * (8 * W + 6) if conv else 8 * W
    fec = flag | conv
    for kind in TC.KINDS:
        assert d._frame_shape(N, h, kind, fec) == (W, R.max_len(W, h, C.CRC_BYTES[kind], R.PARITY[flag]))
        rng = np.random.default_rng(flag + 10 * h + conv + kind)
        pool = np.stack(case_rows(A, flag, h, kind, W, rng))
        cap = len(pool) + 2
        buf = np.concatenate([pool, rng.integers(0, 256, (2, W)).astype(np.uint8)])
        want = host_stage(A, buf, [len(pool)], cap, h, kind, fec)
        same(run_stage(A, torch, d, buf, [len(pool)], cap, N, h, kind, fec), want, ("one group", kind))
        rec = want[1][0, :len(pool)].copy().view(A.FRAME_RS_DTYPE).reshape(-1)
        most = R.max_len(W, h, C.CRC_BYTES[kind], R.PARITY[flag])
        assert set(rec["status"].tolist()) == {R.OK, R.FAILED} | ({R.BAD_LENGTH} if most + 1 < 256 ** h else set())
        assert rec["corrected"].max() >= R.PARITY[flag] // 2
    # three groups, max_frames 4: counts 0, 2 and 9 (clamped to 4)
    pick = pool[rng.choice(len(pool), 12, replace=False)]
    want = host_stage(A, pick, [0, 2, 9], 4, h, kind, fec)
    got = run_stage(A, torch, d, pick, [0, 2, 9], 4, N, h, kind, fec)
    same(got, want, "three groups")
    assert (got[1][0] == POISON).all() and (got[1][1, 2:] == POISON).all() and (got[0][0] == pick[:4]).all()


@pytest.mark.parametrize("flag", TC.FLAGS)
def test_stage_at_the_payload_limit(A, torch, handle, flag):
    """h 2, CRC-32, len 4096: 18 or 19 codewords in a row of exactly n' bytes
    and a full LDS slice, every pattern of tests/rs_cases.py: "ends" corrects
    the row's very last byte beside the guard band, "header" names 4100 data
    bytes, which the row does not hold."""
    d = handle(2)
    P = R.PARITY[flag]
    W = R.frame_size(2 + 4096 + 4, P)
    rng = np.random.default_rng(flag)
    data = bytes(rng.integers(0, 256, 4096, dtype=np.uint8))
    sent = A.rs_frame_encode(data, 2, C.CRC32, flag)
    assert len(sent) == W == {16: 4390, 32: 4710}[P]
    rows = []
    for pattern in TC.PATTERNS:
        row = bytearray(sent)
        TC.corrupt(row, 4102, P, 2, pattern, rng)
        rows.append(np.frombuffer(bytes(row), np.uint8))
    buf = np.stack(rows)
    cap = len(rows)
    want = host_stage(A, buf, [cap], cap, 2, C.CRC32, flag)
    same(run_stage(A, torch, d, buf, [cap], cap, 8 * W, 2, C.CRC32, flag), want)
    rec = dict(zip(TC.PATTERNS, want[1][0].copy().view(A.FRAME_RS_DTYPE).reshape(-1)))
    D = R.codewords(4102, P)
    assert [int(rec[p]["corrected"]) for p in ("none", "one", "t", "parity", "ends")] == [0, D, D * P // 2, D * P // 2,
                                                                                             2 * D]
    for i, p in enumerate(TC.PATTERNS):
        if p not in ("t+1", "header"):
            assert bytes(want[0][0, i]) == sent and rec[p]["status"] == R.OK, p
    assert rec["header"]["status"] == R.BAD_LENGTH and buf[TC.PATTERNS.index("ends"), -1] != sent[-1]


def test_more_rows_than_waves(A, torch, handle):
    """20000 groups of 3 rows, len <= 8: one wave a group, which takes up to
    three rows and reuses its LDS slice. Counts 0 .. 5 (clamped to 3)."""
    d = handle(2)
    flag, h, kind, W, S, cap = R.FLAG16, 1, C.CRC16, 32, 20000, 3
    rng = np.random.default_rng(20000)
    pool = np.stack(case_rows(A, flag, h, kind, W, rng, lengths=(0, 3, 8),
                              patterns=("none", "one", "t", "t+1", "ends")))
    buf = pool[rng.integers(0, len(pool), S * cap)]
    counts = rng.integers(0, 6, S)
    counts[0], counts[1], counts[-1] = 3, 0, 5
    want = host_stage(A, buf, counts, cap, h, kind, flag)
    same(run_stage(A, torch, d, buf, counts, cap, 8 * W, h, kind, flag), want)


# ---- 2. captured behind the scan ---------------------------------------------------------------

def lay(truth, K, Rn, rng):
    """(sym, P) of a batch whose phase 0 carries `truth`, one symbol every Rn
    windows with its tone at 1000 .. 1999; random symbols at 300 .. 599 on the
    other phases, every other tone 1 .. 299: the metric picks phase 0."""
    sym = rng.integers(0, K, truth.size * Rn).astype(np.uint8)
    sym[::Rn] = truth
    P = rng.integers(1, 300, (sym.size, K)).astype(np.float32)
    P[np.arange(sym.size), sym] = rng.integers(300, 600, sym.size)
    P[np.arange(0, sym.size, Rn), truth] = rng.integers(1000, 2000, truth.size)
    return sym, P


def plant_bytes(datas, h, kind, fec, per_codeword):
    """plant() of rs_chain_ref.stream_symbols at one bit a symbol: one wrong
    symbol in each of `per_codeword` bytes of every codeword, the header spared."""
    def plant(f, Sp, rng):
        n, P, out = h + len(datas[f]) + C.CRC_BYTES[kind], R.mode_parity(fec), []
        for j in range(R.codewords(n, P)):
            off = [o for o in R.offsets(n, P, j) if o >= h]
            out += [8 * int(o) + int(rng.integers(8)) for o in rng.choice(off, per_codeword, replace=False)]
        return out
    return plant


def test_capture_behind_the_scan(A, torch, handle):
    """demod_frames_async and the stage in one graph on a side stream, replayed
    after the symbols and powers were rewritten in place: each replay's packed
    rows and records are the host chain's for that content."""
    d = handle(2)
    K, Rn, h, kind, fec, L = 2, 4, 1, C.CRC16, R.FLAG16, 16
    lens = (0, 30, 250, 7)
    N = Z.symbols_for(max(lens), 1, h, kind, fec) + 3
    contents = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        word = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 1, 1], np.uint8)
        datas = [rng.integers(0, 256, m).astype(np.uint8).tobytes() for m in lens]
        truth, _ = H.stream_symbols(A, K, fec, h, kind, datas, N, word, plant_bytes(datas, h, kind, fec, 8), rng)
        sym, P = lay(truth, K, Rn, rng)
        contents.append((sym, P, H.chain(A, sym, P, Rn, word, 1, N, h, kind, fec), datas))
    Wn = len(contents[0][0])
    assert len(contents[1][0]) == Wn
    cap, B = 32, (N + 7) // 8
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_sym, d_mag = torch.zeros(Wn, **u8), torch.zeros(Wn * K, dtype=torch.float32, device="cuda")
    d_hits, d_packed = torch.full((cap * 16,), POISON, **u8), torch.full((cap * B,), POISON, **u8)
    d_res, d_rs = torch.zeros(RES_BYTES, **u8), torch.full((cap * 16,), POISON, **u8)
    d_work = torch.zeros(A.frames_workspace_size(d.cfg, Wn), **u8)

    def enqueue(stream):
        d.frames_async(d_sym, d_mag, Wn, word, 1, N, d_hits, None, d_packed, cap, d_res, d_work, stream=stream)
        d.frames_rs_async(d_packed, d_res, 1, cap, N, h, kind, fec, d_rs, stream=stream)

    def load(sym, P):
        d_sym.copy_(torch.from_numpy(sym))
        d_mag.copy_(torch.from_numpy(P.reshape(-1)))
        for t in (d_packed, d_rs):
            t.fill_(POISON)
        torch.cuda.synchronize()

    def holds(sym, P, want, datas, what):
        hits, before, after, rec, chk, res = want
        nw = len(hits)
        assert 4 <= nw <= cap and chk[2] == datas and int(rec["corrected"].sum()) >= 8 * 5, what
        torch.cuda.synchronize()
        rows = d_packed.cpu().numpy().reshape(cap, B)
        recs = d_rs.cpu().numpy().reshape(cap, 16)
        assert np.array_equal(rows[:nw], after) and (rows[nw:] == POISON).all(), what
        assert recs[:nw].tobytes() == rec.tobytes() and (recs[nw:] == POISON).all(), what

    side = torch.cuda.Stream()
    load(*contents[0][:2])
    with torch.cuda.stream(side):
        enqueue(side.cuda_stream)          # an eager call of the shape first
    holds(*contents[0], "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for k in (1, 0, 1):
        load(*contents[k][:2])
        g.replay()
        holds(*contents[k], ("replay", k))


# ---- 3. refusals ------------------------------------------------------------------------------------

def test_refusals(A, torch, handle):
    """fec of 0, 2, 0x10, 0x31, 0x81 and both parity flags at every device
    entry that takes it; the stage also refuses a mode without a parity flag, a
    NULL or misaligned d_rs and rows narrower than the shortest frame:
    DEMOD_BAD_ARG before any launch, the outputs stay poison. The same calls,
    legal, run in each of the modes they take."""
    lib = A.load_library()
    d = handle(2)
    S, cap, N, L, Wn = 3, 4, 1024, 8, 5000
    rows = S * cap
    u8 = dict(dtype=torch.uint8, device="cuda")

    def poison(nbytes):
        return torch.full((nbytes,), POISON, **u8)
    d_hits, d_res = torch.zeros(rows * 16, **u8), torch.zeros(S * RES_BYTES, **u8)
    d_mag = torch.ones(Wn * 2, dtype=torch.float32, device="cuda")
    d_state = torch.zeros(S * 40, **u8)
    need = max(A.fec_decode_workspace_size(d.cfg, S, cap, N, f) for f in A.RS_CONV_MODES)
    d_rows, d_dec, d_work, d_rs = poison(rows * 128), poison(rows * 16), poison(need), poison(rows * 16 + 4)
    d_check, d_kept, d_body, d_sum = poison(rows * 16), poison(rows * 4), poison(rows * 128), poison(S * 32)
    d_frames, d_bodies, d_rsum = poison(rows * 32), poison(rows * 128), poison(32)
    d_cwork = poison(A.rx_collect_workspace_size(d.cfg, S))
    ph, pm, pr, po, pd, pw = (t.data_ptr() for t in (d_hits, d_mag, d_res, d_rows, d_dec, d_work))
    pc, pk, pb, ps, prs = (t.data_ptr() for t in (d_check, d_kept, d_body, d_sum, d_rs))
    kind = A.DEMOD_CRC16_CCITT_FALSE

    def stage(fec, h=d._h, n=N, rs=prs):
        return lib.demod_frames_rs_async(h, po, pr, S, cap, n, 1, kind, fec, rs, None)

    def decode(fec):
        return lib.demod_frames_decode_async(d._h, ph, pm, Wn, None, pr, S, cap, L, N, 1, kind, fec, po, pd, pw,
                                             d_work.numel(), None)

    def check(fec, n=N):
        return lib.demod_frames_check_coded_async(d._h, ph, po, pr, S, cap, L, n, 1, kind, fec, pc, pk, pb, ps, None)

    def collect(fec):
        return lib.demod_rx_collect_async(d._h, d_state.data_ptr(), ph, pr, pc, pk, pb, ps, S, cap, L, N, 1, kind, fec,
                                          d_frames.data_ptr(), d_bodies.data_ptr(), d_rsum.data_ptr(),
                                          d_cwork.data_ptr(), d_cwork.numel(), None)
    for fec in TC.BAD_MODES + (0x300, 0x301, 0x400):
        assert stage(fec) == decode(fec) == check(fec) == A.DEMOD_BAD_ARG, fec
        if fec:
            assert collect(fec) == A.DEMOD_BAD_ARG, fec
        with pytest.raises(A.DemodError):
            d.frames_coded(np.zeros(8192, np.int16), [0, 1], frame_symbols=N, fec=fec)
    for fec in A.FEC_MODES:
        assert stage(fec) == A.DEMOD_BAD_ARG                    # no parity flag
    for fec in (0x100, 0x200):
        assert decode(fec) == A.DEMOD_BAD_ARG                   # no convolutional code
    assert stage(0x100, rs=None) == A.DEMOD_BAD_ARG and stage(0x100, rs=prs + 2) == A.DEMOD_BAD_ARG
    assert stage(0x100, h=None) == A.DEMOD_BAD_ARG
    assert stage(0x100, n=8 * 18) == A.DEMOD_BAD_ARG and check(0x100, n=8 * 18) == A.DEMOD_BAD_ARG   # W < n'(0) = 19
    assert stage(0x200, n=8 * 34) == A.DEMOD_BAD_ARG and stage(0x200, n=8 * 35) == A.DEMOD_OK
    assert stage(0x100, n=8 * 4391) == A.DEMOD_BAD_ARG          # max_len would pass DEMOD_MAX_FRAME_PAYLOAD
    with A.Demodulator(n=1024, hop=256, freqs=(1500.0, 2250.0, 3000.0)) as k3:
        assert stage(0x141, h=k3._h) == A.DEMOD_BAD_ARG         # a coded mode needs K = 2^bits
        assert stage(0x100, h=k3._h, n=512) == A.DEMOD_OK        # the plain parity mode does not
    torch.cuda.synchronize()
    for t in (d_rows, d_dec, d_work, d_rs, d_check, d_kept, d_body, d_sum, d_frames, d_bodies, d_rsum, d_cwork):
        assert bool((t == POISON).all()), "a refused call wrote"
    # and the same calls, legal, run: three empty groups
    for fec in A.RS_MODES:
        if fec & 0x300:
            assert stage(fec) == A.DEMOD_OK, fec
        if fec & 0xFF:
            assert decode(fec) == A.DEMOD_OK, fec
        assert check(fec) == collect(fec) == A.DEMOD_OK, fec
    torch.cuda.synchronize()
    assert not d_sum.cpu().numpy().any()
    for t in (d_rows, d_dec, d_rs, d_check, d_kept, d_body):
        assert bool((t == POISON).all())


def test_refusals_receiver_and_transmitter(A, torch, handle):
    """The same bad values at demod_rx_create, demod_tx_create,
    demod_tx_encode_async and demod_tx_modulate_async, called directly: no
    handle, DEMOD_BAD_ARG, the outputs stay poison. In the 20 modes the same
    calls run."""
    lib = A.load_library()
    d = handle(2)
    S, word = 2, [0, 1, 1, 0, 1]
    rx_base = dict(sync=word, max_errors=0, frame_symbols=1024, len_bytes=1, crc=C.CRC16, max_frames=4,
                   ring_windows=2 * 1029 * 4)
    tx_base = dict(sync=word, len_bytes=1, crc=C.CRC16, max_len=16, ring_symbols=8192, max_frames=2, max_samples=2880)
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_state, d_ring = torch.zeros(S * 40, **u8), torch.full((S * 8192,), POISON, **u8)
    d_rec, d_place = torch.zeros(S * 2 * 8, **u8), torch.full((S * 2 * 16,), POISON, **u8)
    d_count = torch.zeros(S, dtype=torch.int32, device="cuda")
    d_pcm = torch.full((S * 2880,), -1, dtype=torch.int16, device="cuda")
    d_work = torch.full((4096,), POISON, **u8)

    def create(fn, cfgs):
        err = ctypes.c_int(0)
        h = fn(ctypes.byref(d.cfg), ctypes.byref(cfgs), S, ctypes.byref(err))
        return h, err.value

    def encode(x):
        return lib.demod_tx_encode_async(d._h, ctypes.byref(x), d_state.data_ptr(), d_ring.data_ptr(),
                                         d_rec.data_ptr(), d_count.data_ptr(), None, 0, S, d_place.data_ptr(), None)

    def modulate(x):
        return lib.demod_tx_modulate_async(d._h, ctypes.byref(x), d_state.data_ptr(), d_ring.data_ptr(),
                                           d_count.data_ptr(), S, d_pcm.data_ptr(), d_work.data_ptr(),
                                           d_work.numel(), None)
    for fec in TC.BAD_MODES[1:] + (0x300, 0x301, 0x400):       # 0 is "no code" to both, as before
        h, err = create(lib.demod_rx_create, A.make_rx_cfg(fec=fec, **rx_base))
        assert not h and err == A.DEMOD_BAD_ARG, fec
        x = A.make_tx_cfg(fec=fec, **tx_base)
        h, err = create(lib.demod_tx_create, x)
        assert not h and err == A.DEMOD_BAD_ARG, fec
        assert encode(x) == A.DEMOD_BAD_ARG and modulate(x) == A.DEMOD_BAD_ARG, fec
        with pytest.raises(A.DemodError):
            A.Receiver(S, A.make_rx_cfg(fec=fec, **rx_base), n=1024, hop=256, freqs=T.loop_tones(2))
        with pytest.raises(A.DemodError):
            A.Transmitter(S, x, n=1024, hop=256, freqs=T.loop_tones(2))
    torch.cuda.synchronize()
    assert bool((d_ring == POISON).all()) and bool((d_place == POISON).all()) and bool((d_pcm == -1).all())
    for fec in A.RS_MODES:
        x = A.make_tx_cfg(fec=fec, **tx_base)
        assert encode(x) == A.DEMOD_OK, fec                     # no frames: nothing queued
        with A.Receiver(S, A.make_rx_cfg(fec=fec, **rx_base), n=1024, hop=256, freqs=T.loop_tones(2)) as rx:
            assert rx.sizes["max_len"] == H.max_len(A, 1024, 1, 1, C.CRC16, fec)
        with A.Transmitter(S, x, n=1024, hop=256, freqs=T.loop_tones(2)) as tx:
            assert tx.sizes["max_symbols"] == 5 + Z.span(16, 1, 1, C.CRC16, fec)
    torch.cuda.synchronize()
    assert bool((d_ring == POISON).all())


# ---- 4. the one-shot call and the receiver ------------------------------------------------------------

E2E = {0x100: dict(K=2, h=1, kind=C.CRC16, lens=(0, 30, 250, 7)),
       0x251: dict(K=8, h=2, kind=C.CRC32, lens=(0, 40, 300, 9))}
E2E_L = 16
_E2E = {}


def e2e_case(A, fec):
    """Four frames of the mode as FSK (n 1024), with planted wrong symbols: at
    0x100 eight wrong bytes in every codeword; at 0x251 a run of 10 wrong
    symbols in the second interleaver block of the two longer frames, which
    the Viterbi decoder alone does not take."""
    if fec not in _E2E:
        c = E2E[fec]
        K, h, kind, lens = c["K"], c["h"], c["kind"], c["lens"]
        bits = F.bits_per_symbol(K)
        rng = np.random.default_rng(fec)
        word = rng.integers(0, K, E2E_L).astype(np.uint8)
        datas = [rng.integers(0, 256, m).astype(np.uint8).tobytes() for m in lens]
        N = Z.symbols_for(max(lens), bits, h, kind, fec) + 3
        if fec & 0xFF:
            def plant(f, Sp, rng):
                return list(range(100, 110)) if Sp > 300 else []
        else:
            plant = plant_bytes(datas, h, kind, fec, 8)
        truth, at = H.stream_symbols(A, K, fec, h, kind, datas, N, word, plant, rng)
        _E2E[fec] = dict(c, bits=bits, word=word, datas=datas, N=N, at=at,
                         pcm=H.pcm_of(T.loop_tones(K), truth, 7 + fec))
    return _E2E[fec]


@pytest.mark.parametrize("fec", sorted(E2E))
def test_frames_coded(A, torch, handle, fec):
    """demod_frames_coded at 0x100 (K 2) and 0x251 (K 8), hop 256: kept hits,
    lengths, bodies and summary equal the host chain (scan, soft values and
    Viterbi decode, outer decode, check with the span of n') on the device
    detector's own (sym, P), and the frames sent come back although their rows
    reach the outer code wrong."""
    c = e2e_case(A, fec)
    d = handle(c["K"])
    K, h, kind, N, word, x = c["K"], c["h"], c["kind"], c["N"], c["word"], c["pcm"]
    Wn = (len(x) - 1024) // 256 + 1
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_pcm = torch.from_numpy(x).cuda()
    d_sym, d_mag = torch.empty(Wn, **u8), torch.empty(Wn * K, dtype=torch.float32, device="cuda")
    d.batch_async(d_pcm, Wn, d_sym, d_mag)
    torch.cuda.synchronize()
    sym, P = d_sym.cpu().numpy(), d_mag.cpu().numpy().reshape(Wn, K)
    hits, before, after, rec, chk, res = H.chain(A, sym, P, 4, word, 1, N, h, kind, fec)
    check, kept, bodies, summ = chk
    summ = dict(zip(summ.dtype.names, summ.tolist()))
    assert bodies == c["datas"] and [int(hits["window"][i]) for i in kept] == [4 * a for a in c["at"]]
    assert int(rec["corrected"][kept].sum()) > 0 and not np.array_equal(before, after)   # the outer code did it
    for pcm in (x, d_pcm):
        g_hits, lengths, body, g_res, summary = d.frames_coded(pcm, word, max_errors=1, frame_symbols=N,
                                                                len_bytes=h, crc=kind, fec=fec)
        assert body == bodies and lengths.tolist() == [len(b) for b in bodies]
        assert g_hits.tobytes() == hits[kept].tobytes() and summary == summ
        assert g_res["n_written"] == res["n_written"] == len(hits)


@pytest.mark.parametrize("fec", sorted(E2E))
def test_rx_push(A, torch, handle, fec):
    """demod_rx_push in the same two modes, two streams (the second delayed by
    100 samples), in packets of 48000 frames, which split every frame but the
    shortest: each stream's frames are demod_frames_coded's on its recording."""
    c = e2e_case(A, fec)
    d = handle(c["K"])
    K, h, kind, N, word, x = c["K"], c["h"], c["kind"], c["N"], c["word"], c["pcm"]
    rng = np.random.default_rng(1)
    recs = [x, np.concatenate([rng.integers(-300, 301, 100).astype(np.int16), x])]
    want = []
    for r in recs:
        g_hits, _, body, _, _ = d.frames_coded(r, word, max_errors=1, frame_symbols=N, len_bytes=h, crc=kind, fec=fec)
        want.append([(int(hh["window"]), int(hh["errors"]), b) for hh, b in zip(g_hits, body)])
        assert [b for _, _, b in want[-1]] == c["datas"]
    ring = (len(recs[1]) - 1024) // 256 + 1 + 64
    rxcfg = A.make_rx_cfg(word, 1, N, h, kind, fec, 8, ring)
    got = [[], []]
    with A.Receiver(2, rxcfg, n=1024, hop=256, freqs=T.loop_tones(K)) as rx:
        assert rx.sizes["max_len"] == H.max_len(A, N, c["bits"], h, kind, fec)
        for at in range(0, len(recs[1]), 48000):
            fr, bodies, summ = rx.push([r[at:at + 48000] if at < len(r) else None for r in recs])
            assert summ["n_frames"] == len(fr)
            for f, b in zip(fr, bodies):
                got[int(f["stream"])].append((int(f["window"]), int(f["errors"]), b))
    assert got == want


# ---- 5. the transmitter ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fec,K", [(0x100, 2), (0x200, 8), (0x101, 2), (0x261, 8), (0x151, 8)])
def test_transmitter_symbols(A, torch, fec, K):
    """demod_tx_encode_async's ring symbols equal the host
    demod_tx_frame_symbols: lengths 0, 1, the last with one codeword, the
    first with two, one with three unequal codewords; two streams in opposite
    orders, gap 0 and poison behind the frames."""
    n, S, h, kind = 256, 2, 2, C.CRC16
    P = R.mode_parity(fec)
    lens = TC.edge_lengths(h, 2, P)[:5]
    word = (np.arange(11) * 5) % K
    rng = np.random.default_rng(fec + K)
    datas = [rng.integers(0, 256, ln).astype(np.uint8).tobytes() for ln in lens]
    bits = F.bits_per_symbol(K)
    counts = [11 + Z.span(ln, bits, h, kind, fec) for ln in lens]
    ring = sum(counts) + 9
    x = A.make_tx_cfg(word, h, kind, fec, max(lens), 0, (0,), 8000, 0, 0, ring, len(lens), 2880)
    want = [A.tx_frame_symbols(x, K, data) for data in datas]
    assert [len(w) for w in want] == counts
    records = np.zeros((S, len(lens)), T.RECORD_DTYPE)
    blob, at = b"", []
    for data in datas:
        at.append(len(blob))
        blob += data
    orders = [list(range(len(lens))), list(range(len(lens) - 1, -1, -1))]
    for s in range(S):
        for i, f in enumerate(orders[s]):
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
        for i, f in enumerate(orders[s]):
            start, cnt = int(place["start"][s, i]), int(place["symbols"][s, i])
            assert cnt == counts[f] and start == sum(counts[g] for g in orders[s][:i])
            bad = np.flatnonzero(got[s, start:start + cnt] != want[f])
            assert bad.size == 0, (hex(fec), K, s, lens[f], bad[:6].tolist())
        assert (got[s, sum(counts):] == POISON).all()


@pytest.mark.parametrize("fec,length", [(0x100, 300), (0x211, 230)])
def test_loop_into_the_receiver(A, torch, fec, length):
    """demod_tx_send and demod_tx_pull into demod_rx_push at 8 tones, one plain
    and one coded parity mode, frames of two codewords and a short one, two
    streams at two sample offsets: every frame comes back, in order."""
    K, S, L, h, kind, n, hop, packet = 8, 2, 16, 2, C.CRC32, 1024, 256, 48000
    assert R.codewords(h + length + 4, R.mode_parity(fec)) == 2
    rng = np.random.default_rng(fec)
    word = rng.integers(0, K, L).astype(np.uint8)
    datas = [rng.integers(0, 256, m).astype(np.uint8).tobytes() for m in (length, 5)]
    gap = 3
    per = [L + Z.span(len(dd), 3, h, kind, fec) + gap for dd in datas]
    N = Z.symbols_for(length, 3, h, kind, fec)
    total = -(-(3 + sum(per) + N + 8) * n // packet) * packet
    x = A.make_tx_cfg(word, h, kind, fec, length, gap, (0, 1), 8000, 400, 77, sum(per) + 5, len(datas), packet)
    freqs = T.loop_tones(K)
    pcm = [[] for _ in range(S)]
    with A.Transmitter(S, x, n=n, hop=hop, freqs=freqs) as tx:
        for at in range(0, total, packet):
            if at == packet:
                accepted, place = tx.send([(s, dd) for s in range(S) for dd in datas])
                assert accepted == S * len(datas) and (place["status"] == T.OK).all()
                assert place["symbols"].tolist() == [p - gap for p in per] * S
            out = tx.pull(packet)
            for s in range(S):
                pcm[s].append(out[s])
    pcm = [np.concatenate(p)[drop:] for p, drop in zip(pcm, (0, 100))]
    rxcfg = A.make_rx_cfg(word, 2, N, h, kind, fec, 8, total // hop + 64)
    got = [[] for _ in range(S)]
    with A.Receiver(S, rxcfg, n=n, hop=hop, freqs=freqs) as rx:
        for at in range(0, total, packet):
            fr, bodies, _ = rx.push([p[at:at + packet] if at < len(p) else None for p in pcm])
            for f, b in zip(fr, bodies):
                got[int(f["stream"])].append(b)
    assert got == [datas] * S
