"""Erasure decoding on the GPU (include/demod.h "erasure decoding"): the
stage's second instantiation (frames_rs.hip) on rows and masks uploaded from
the host against demod_rs_frame_decode_erasures, bit for bit in the rows and in
both records; an all-zero mask against demod_frames_rs_async; the producer
(frames_erasures.hip) against demod_soft_bits and demod_soft_erasures from
crafted powers; guard bands at two poisons; scan, producer, stage and check in
one captured graph; demod_frames_coded and demod_rx_push through a dropout; and
the refusals of the device entries.
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
import rs_cases as RC
import rs_chain_ref as H
import rs_erasure_cases as EC
import rs_ref as R
import tx_ref as T
from gpu_support import handle_fixture, results_bytes, same as whole_same, torch  # noqa: F401

pytestmark = pytest.mark.gpu

RES_BYTES = F.RESULT_DTYPE.itemsize
GUARD = 4096
POISONS = (0xFF, 0x5A)


# handle(K, hop): one Demodulator (n 1024) per K and hop, closed with the module.
handle = handle_fixture(lambda A, K, hop=256: A.Demodulator(n=1024, hop=hop, freqs=T.loop_tones(K)))


def as_i64(torch, words):
    return torch.from_numpy(np.ascontiguousarray(words, np.uint64).view(np.int64).reshape(-1).copy())


def host_stage(A, rows, masks, counts, max_frames, h, kind, fec, poison):
    """demod_rs_frame_decode_erasures over rows i < min(count_g, max_frames) of
    every group; the other rows stay, their records stay poison."""
    n_groups = len(counts)
    out = rows.copy().reshape(n_groups, max_frames, -1)
    masks = masks.reshape(n_groups, max_frames, -1)
    rec = np.full((n_groups, max_frames, 16), poison, np.uint8)
    erec = np.full((n_groups, max_frames, 16), poison, np.uint8)
    memo = {}
    for g in range(n_groups):
        for i in range(min(int(counts[g]), max_frames)):
            key = out[g, i].tobytes() + masks[g, i].tobytes()
            if key not in memo:
                got, r, e, _ = A.rs_frame_decode(out[g, i], h, kind, fec, erase=masks[g, i])
                memo[key] = (got, np.array([tuple(r[f] for f in A.FRAME_RS_DTYPE.names)], A.FRAME_RS_DTYPE),
                             np.array([tuple(e[f] for f in A.FRAME_ERASE_DTYPE.names)], A.FRAME_ERASE_DTYPE))
            out[g, i] = memo[key][0]
            rec[g, i] = memo[key][1].view(np.uint8)
            erec[g, i] = memo[key][2].view(np.uint8)
    return out, rec, erec


def run_stage(A, torch, d, rows, masks, counts, max_frames, N, h, kind, fec, poison=POISONS[0]):
    """The stage on rows [n_groups * max_frames][W] and masks [..][Wm] between
    guard bands: (rows, records, erasure records) after it, the guards and the
    inputs checked."""
    n_groups, W = len(counts), rows.shape[-1]
    Wm = A.mask_words(W)
    n = n_groups * max_frames
    d_rows, chk_rows = G.guarded(torch, n * W, torch.uint8, GUARD, GUARD, poison)
    d_rs, chk_rs = G.guarded(torch, n * 16, torch.uint8, GUARD, GUARD, poison)
    d_erec, chk_erec = G.guarded(torch, n * 16, torch.uint8, GUARD, GUARD, poison)
    d_rows.copy_(torch.from_numpy(np.array(rows, np.uint8).reshape(-1)))
    words = np.ascontiguousarray(masks, np.uint64).reshape(-1)
    assert words.size == n * Wm
    d_erase = as_i64(torch, words).cuda()
    res = results_bytes(counts).reshape(-1)
    d_res = torch.from_numpy(res.copy()).cuda()
    d.frames_rs_erasures_async(d_rows, d_erase, d_res, n_groups, max_frames, N, h, kind, fec, d_rs, d_erec)
    for chk in (chk_rows, chk_rs, chk_erec):
        chk(written=False)
    assert d_res.cpu().numpy().tobytes() == res.tobytes(), "the results were written to"
    assert d_erase.cpu().numpy().tobytes() == words.view(np.int64).tobytes(), "the masks were written to"
    shape = (n_groups, max_frames)
    return (d_rows.cpu().numpy().reshape(*shape, W), d_rs.cpu().numpy().reshape(*shape, 16),
            d_erec.cpu().numpy().reshape(*shape, 16))


same = functools.partial(whole_same, names=("rows", "records", "erasure records"))


def planted_rows(A, flag, h, kind, length, W, rng):
    """Rows of W bytes and their masks: the frame of `length` data bytes under
    every round of tests/rs_erasure_cases.py, flags past n' included; a header
    of max_len + 1 between them; two random rows with random masks."""
    P, c = R.PARITY[flag], C.CRC_BYTES[kind]
    n = h + length + c
    D = R.codewords(n, P)
    sent = A.rs_frame_encode(bytes(rng.integers(0, 256, length, dtype=np.uint8)), h, kind, flag)
    assert len(sent) <= W
    rows, masks = [], []
    for plan in EC.rounds(P, D):
        row = bytearray(sent + bytes(rng.integers(0, 256, W - len(sent), dtype=np.uint8)))
        flags = np.zeros(W, bool)
        flags[len(sent):] = rng.integers(0, 2, W - len(sent)).astype(bool)
        EC.plant(row, flags, n, P, h, rng, plan)
        rows.append(np.frombuffer(bytes(row), np.uint8))
        masks.append(A.pack_mask(flags, W))
    most = R.max_len(W, h, c, P)
    if most + 1 < 256 ** h:
        rows.insert(1, np.frombuffer((most + 1).to_bytes(h, "big") + bytes(rng.integers(0, 256, W - h, dtype=np.uint8)),
                                     np.uint8))
        masks.insert(1, A.pack_mask(rng.integers(0, 2, W).astype(bool), W))
    for _ in range(2):
        rows.append(rng.integers(0, 256, W).astype(np.uint8))
        masks.append(A.pack_mask(rng.random(W) < 0.05, W))
    return np.stack(rows), np.stack(masks)


# ---- 1. the stage against the host decoder ---------------------------------------------------

@pytest.mark.parametrize("flag,h,kind,length,pad", [
    (R.FLAG16, 2, C.CRC32, 4 * 239 + 17, 5),     # D = 5: a second pass of the slot loop with one live slot
    (R.FLAG32, 2, C.CRC32, 500, 9),              # D = 3 at P = 32
    (R.FLAG16, 1, C.CRC16, 40, 4),               # n' = 59 in rows of 63 bytes: one mask word
    (R.FLAG16, 1, C.CRC16, 50, 0),               # n' = 69: crosses a 64-byte word, W = n'
])
def test_stage_against_host(A, torch, handle, flag, h, kind, length, pad):
    """Every combination of tests/rs_erasure_cases.py in every codeword, a
    BAD_LENGTH row between good ones and random rows, as one group with two rows
    past the count; then three groups with counts 0, 2 and max_frames + 5."""
    d = handle(2)
    P = R.PARITY[flag]
    W = R.frame_size(h + length + C.CRC_BYTES[kind], P) + pad
    assert W % 64 != 0
    N = 8 * W
    rng = np.random.default_rng(flag + length)
    rows, masks = planted_rows(A, flag, h, kind, length, W, rng)
    cap = len(rows) + 2
    buf = np.concatenate([rows, rng.integers(0, 256, (2, W)).astype(np.uint8)])
    msk = np.concatenate([masks, np.full((2, masks.shape[1]), 2 ** 64 - 1, np.uint64)])
    want = host_stage(A, buf, msk, [len(rows)], cap, h, kind, flag, POISONS[0])
    same(run_stage(A, torch, d, buf, msk, [len(rows)], cap, N, h, kind, flag), want, "one group")
    er = want[2][0, :len(rows)].copy().view(A.FRAME_ERASE_DTYPE).reshape(-1)
    rs = want[1][0, :len(rows)].copy().view(A.FRAME_RS_DTYPE).reshape(-1)
    assert er["used"].sum() > 0 and er["fallback"].sum() > 0 and rs["failed"].sum() > 0
    if h == 1:
        assert R.BAD_LENGTH in rs["status"].tolist()
    pick = rng.choice(len(rows), 12, replace=len(rows) < 12)
    want = host_stage(A, rows[pick], masks[pick], [0, 2, 9], 4, h, kind, flag, POISONS[1])
    got = run_stage(A, torch, d, rows[pick], masks[pick], [0, 2, 9], 4, N, h, kind, flag, POISONS[1])
    same(got, want, "three groups")
    assert (got[2][0] == POISONS[1]).all() and (got[2][1, 2:] == POISONS[1]).all()
    assert (got[0][0] == rows[pick][:4]).all() and (got[0][1, 2:] == rows[pick][6:8]).all()


def test_stage_at_the_payload_limit(A, torch, handle):
    """One row of exactly n' = 4710 bytes: P = 32, D = 19, a full LDS slice and 74 mask words."""
    d = handle(2)
    flag, P, h, kind, W = R.FLAG32, 32, 2, C.CRC32, 4710
    rng = np.random.default_rng(4710)
    sent = A.rs_frame_encode(bytes(rng.integers(0, 256, 4096, dtype=np.uint8)), h, kind, flag)
    row, flags = bytearray(sent), np.zeros(W, bool)
    EC.plant(row, flags, 4102, P, h, rng, EC.combos(P))
    flags[-1] = True
    buf, msk = np.frombuffer(bytes(row), np.uint8)[None, :], A.pack_mask(flags, W)[None, :]
    assert msk.shape == (1, 74)
    want = host_stage(A, buf, msk, [1], 1, h, kind, flag, POISONS[0])
    same(run_stage(A, torch, d, buf, msk, [1], 1, 8 * W, h, kind, flag), want)
    er = want[2][0, 0].copy().view(A.FRAME_ERASE_DTYPE)[0]
    assert er["used"] >= 5 and er["fallback"] >= 2


def test_four_branches_in_one_pass(A, torch, handle):
    """P = 16, D = 4: the four codewords of one pass are clean, accepted by the
    first attempt, accepted by the fallback and failed."""
    d = handle(2)
    flag, P, h, kind, length = R.FLAG16, 16, 2, C.CRC16, 800
    n = h + length + 2
    assert R.codewords(n, P) == 4
    rng = np.random.default_rng(4)
    sent = A.rs_frame_encode(bytes(rng.integers(0, 256, length, dtype=np.uint8)), h, kind, flag)
    W = len(sent) + 3
    row, flags = bytearray(sent + bytes(3)), np.zeros(W, bool)
    plan = {1: (10, 3, True), 2: (4, 7, False), 3: (1, 12, False)}      # f, e, the flagged bytes wrong
    for j, (f, e, wrong) in plan.items():
        off = [o for o in R.offsets(n, P, j) if o >= h]
        at = rng.choice(off, f + e, replace=False)
        flags[at[:f]] = True
        for o in (at if wrong else at[f:]):
            row[o] ^= int(rng.integers(1, 256))
    buf, msk = np.frombuffer(bytes(row), np.uint8)[None, :], A.pack_mask(flags, W)[None, :]
    want = host_stage(A, buf, msk, [1], 1, h, kind, flag, POISONS[0])
    same(run_stage(A, torch, d, buf, msk, [1], 1, 8 * W, h, kind, flag), want)
    assert want[2][0, 0].copy().view(A.FRAME_ERASE_DTYPE)[0].tolist() == (15, 1, 2, 0)
    assert want[1][0, 0].copy().view(A.FRAME_RS_DTYPE)[0].tolist() == (R.FAILED, 4, 13 + 7, 1)


def test_a_wave_walks_more_than_one_row(A, torch, handle):
    """8193 groups of 3 rows: one wave a group (16384 / 8193), which takes up
    to three rows and reuses its LDS slice, masks included. Counts 0 .. 5."""
    d = handle(2)
    flag, h, kind, W, S, cap = R.FLAG16, 1, C.CRC16, 40, 8193, 3
    rng = np.random.default_rng(8193)
    pool, pmask = [], []
    for length in (0, 9, 21):
        r, m = planted_rows(A, flag, h, kind, length, W, rng)
        pool.append(r)
        pmask.append(m)
    pool, pmask = np.concatenate(pool), np.concatenate(pmask)
    pick = rng.integers(0, len(pool), S * cap)
    counts = rng.integers(0, 6, S)
    counts[0], counts[1], counts[-1] = 3, 0, 5
    want = host_stage(A, pool[pick], pmask[pick], counts, cap, h, kind, flag, POISONS[0])
    same(run_stage(A, torch, d, pool[pick], pmask[pick], counts, cap, 8 * W, h, kind, flag), want)


# ---- 2. an all-zero mask is the plain stage -----------------------------------------------------

@pytest.mark.parametrize("flag", RC.FLAGS)
def test_zero_mask_is_the_plain_stage(A, torch, handle, flag):
    d = handle(2)
    h, kind, W = 2, C.CRC16, 800
    P = R.PARITY[flag]
    rng = np.random.default_rng(flag)
    rows = []
    for length in RC.edge_lengths(h, 2, P)[:5]:
        sent = A.rs_frame_encode(bytes(rng.integers(0, 256, length, dtype=np.uint8)), h, kind, flag)
        for pattern in RC.PATTERNS:
            row = bytearray(sent + bytes(rng.integers(0, 256, W - len(sent), dtype=np.uint8)))
            RC.corrupt(row, h + length + 2, P, h, pattern, rng)
            rows.append(np.frombuffer(bytes(row), np.uint8))
    rows.append(rng.integers(0, 256, W).astype(np.uint8))
    buf = np.stack(rows)
    cap = len(rows)
    zero = np.zeros((cap, A.mask_words(W)), np.uint64)
    got = run_stage(A, torch, d, buf, zero, [cap], cap, 8 * W, h, kind, flag)
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_rows = torch.from_numpy(buf.reshape(-1).copy()).cuda()
    d_rs = torch.full((cap * 16,), POISONS[0], **u8)
    d_res = torch.from_numpy(results_bytes([cap]).reshape(-1).copy()).cuda()
    d.frames_rs_async(d_rows, d_res, 1, cap, 8 * W, h, kind, flag, d_rs)
    torch.cuda.synchronize()
    assert np.array_equal(got[0][0], d_rows.cpu().numpy().reshape(cap, W))
    assert np.array_equal(got[1][0], d_rs.cpu().numpy().reshape(cap, 16))
    assert (got[2] == 0).all()
    assert not np.array_equal(got[0][0], buf)          # something was corrected


# ---- 3. the producer --------------------------------------------------------------------------------

def host_masks(A, P, windows, counts, cap, first, L, Rn, N, level, poison_word):
    """demod_soft_bits and demod_soft_erasures over rows i < min(count_g, cap)."""
    Wn, K = P.shape
    bits = F.bits_per_symbol(K)
    B = (N * bits + 7) // 8
    soft = X.soft_bits(P)
    out = np.full((len(counts), cap, A.mask_words(B)), poison_word, np.uint64)
    for g in range(len(counts)):
        base = min(int(first[g]), Wn) if first is not None else 0
        for i in range(min(int(counts[g]), cap)):
            out[g, i] = A.soft_erasures(X.row_soft(soft, Wn, base, int(windows[g, i]), L, Rn, N), level, B)
    return out


@pytest.mark.parametrize("K", (2, 4, 8, 16))
@pytest.mark.parametrize("hop", (1024, 256))
def test_producer_against_host(A, torch, handle, K, hop):
    """Crafted powers: zero, equal, NaN and infinite windows (q = 0), weak and
    strong ones; hits whose symbols run past n_windows and one at or past it;
    with and without a segment table; levels 1 and 127; both poisons. Rows and
    mask words of rows >= the count are untouched."""
    d = handle(K, hop)
    Rn, L, bits = 1024 // hop, 5, F.bits_per_symbol(K)
    N = {1: 1035, 2: 531, 3: 347, 4: 261}[bits]            # B > 64 bytes, N bits not a multiple of 8
    B = (N * bits + 7) // 8
    Wm = A.mask_words(B)
    Wn = (L + N) * Rn + 700
    rng = np.random.default_rng(K + hop)
    P = (rng.random((Wn, K), dtype=np.float32) ** 3 * 1000).astype(np.float32)
    strong = rng.random(Wn) < 0.5
    P[strong, rng.integers(0, K, Wn)[strong]] += 5000
    special = rng.choice(Wn, 80, replace=False)
    P[special[:20]] = 0.0
    P[special[20:40]] = 7.0
    P[special[40:60], 0] = np.nan
    P[special[60:80]] = np.inf
    few = np.concatenate([special[::8], np.arange(40)])
    assert np.array_equal(X.soft_bits(P[few]), np.stack([A.soft_bits(P[w]) for w in few]))
    assert (X.soft_bits(P[special[:40]]) == 0).all() and (X.soft_bits(P[special[60:]]) == 0).all()
    cap = 4
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_mag, chk_mag = G.guarded(torch, Wn * K, torch.float32, GUARD, GUARD, POISONS[0])
    d_mag.copy_(torch.from_numpy(P.reshape(-1)))
    mag_bytes = P.tobytes()
    for first, counts, poison in ((None, [3], POISONS[0]), (np.array([0, 300, Wn + 9], np.uint64), [2, 9, 1], POISONS[1])):
        S = len(counts)
        # windows relative to the base: inside, running past n_windows, at and past n_windows
        windows = np.array([[0, 900, Wn, 33], [7, 850, Wn - 1, 123], [0, 1, 2, 3]][:S], np.uint64)
        hits = np.zeros((S, cap), A.FRAME_HIT_DTYPE)
        hits["window"] = windows
        d_hits = torch.from_numpy(hits.view(np.uint8).reshape(-1).copy()).cuda()
        d_res = torch.from_numpy(results_bytes(counts).reshape(-1).copy()).cuda()
        d_first = as_i64(torch, first).cuda() if first is not None else None
        for level in (1, 127):
            d_bytes, chk = G.guarded(torch, S * cap * Wm * 8, torch.uint8, GUARD, GUARD, poison)
            d_erase = d_bytes.view(torch.int64)
            d.frames_erasures_async(d_hits, d_mag, Wn, d_first, d_res, S, cap, L, N, level, d_erase)
            chk(written=False)
            got = d_erase.cpu().numpy().view(np.uint64).reshape(S, cap, Wm)
            word = int.from_bytes(bytes([poison]) * 8, "little")
            want = host_masks(A, P, windows, counts, cap, first, L, Rn, N, level, word)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (K, hop, level, first is not None, bad[:4].tolist())
            live = want[0, 0]
            assert (int(live[-1]) >> ((B - 1) & 63)) & 1 and int(live[-1]) >> (((B - 1) & 63) + 1) == 0
            # a row whose hit is at or past n_windows: every byte flagged, and only the row's bytes
            gone = want[0, 2] if first is None else want[2, 0]
            full = E_full(B, Wm)
            assert gone.tolist() == full
        chk_mag(written=False)
    assert d_mag.cpu().numpy().tobytes() == mag_bytes


def test_producer_at_the_widest_row(A, torch, handle):
    """B = 4710, the widest row any mode takes (the fec-0 row stops at 4102 bytes):
    74 mask words a row; one row inside the batch and one whose symbols run past it."""
    d = handle(2, 1024)
    L, N, level, cap = 5, 8 * 4710, 16, 2
    B, Wm = 4710, 74
    assert A.mask_words(B) == Wm
    Wn = L + N + 50
    rng = np.random.default_rng(4710)
    P = (rng.random((Wn, 2), dtype=np.float32) ** 3 * 1000).astype(np.float32)
    P[rng.random(Wn) < 0.2] = 3.0
    windows = np.array([[0, 90]], np.uint64)
    hits = np.zeros((1, cap), A.FRAME_HIT_DTYPE)
    hits["window"] = windows
    d_mag, chk_mag = G.guarded(torch, Wn * 2, torch.float32, GUARD, GUARD, POISONS[0])
    d_mag.copy_(torch.from_numpy(P.reshape(-1)))
    d_hits = torch.from_numpy(hits.view(np.uint8).reshape(-1).copy()).cuda()
    d_res = torch.from_numpy(results_bytes([2]).reshape(-1).copy()).cuda()
    d_bytes, chk = G.guarded(torch, cap * Wm * 8, torch.uint8, GUARD, GUARD, POISONS[1])
    d.frames_erasures_async(d_hits, d_mag, Wn, None, d_res, 1, cap, L, N, level, d_bytes.view(torch.int64))
    chk(written=False)
    chk_mag(written=False)
    got = d_bytes.cpu().numpy().view(np.uint64).reshape(1, cap, Wm)
    want = host_masks(A, P, windows, [2], cap, None, L, 1, N, level, 0)
    assert np.array_equal(got, want)
    flagged = [sum(bin(int(w)).count("1") for w in want[0, i]) for i in range(cap)]
    assert 0 < flagged[0] < B and 0 < flagged[1] < B
    # the second row's last 40 symbols lie past n_windows: its last five bytes are flagged whatever the powers say
    tail = (1 << (B - 64 * 73)) - 1
    assert int(want[0, 1, -1]) & (tail ^ (tail >> 5)) == tail ^ (tail >> 5)


def E_full(B, Wm):
    return [(1 << min(64, B - 64 * w)) - 1 for w in range(Wm)]


# ---- 4. a captured graph of scan -> producer -> stage -> check ------------------------------------

def lay(truth, lost, K, Rn, rng):
    """(sym, P) of a batch whose phase 0 carries `truth`, one symbol every Rn
    windows with its tone at 1000 .. 1999 (random symbols at 300 .. 599 on the
    other phases, every other tone 1 .. 299); the symbols listed in `lost` are
    a dropout: every tone 5, the decision 0."""
    sym = rng.integers(0, K, truth.size * Rn).astype(np.uint8)
    sym[::Rn] = truth
    P = rng.integers(1, 300, (sym.size, K)).astype(np.float32)
    P[np.arange(sym.size), sym] = rng.integers(300, 600, sym.size)
    P[np.arange(0, sym.size, Rn), truth] = rng.integers(1000, 2000, truth.size)
    for s in lost:
        sym[s * Rn:(s + 1) * Rn] = 0
        P[s * Rn:(s + 1) * Rn] = 5.0
    return sym, P


def dropout_stream(A, K, fec, h, kind, lens, N, word, rng, which=1, first_byte=20, n_bytes=12):
    """Frames whose data is all 0xFF; frame `which` loses the symbols of
    n_bytes consecutive row bytes from first_byte on. Returns (the symbols, the
    words' symbol indices, the lost symbols, the frames' data)."""
    bits = F.bits_per_symbol(K)
    datas = [bytes([0xFF]) * m for m in lens]
    truth, at = H.stream_symbols(A, K, fec, h, kind, datas, N, word, lambda f, Sp, r: [], rng)
    s0 = at[which] + len(word) + (8 * first_byte) // bits
    lost = list(range(s0, s0 + (8 * n_bytes + bits - 1) // bits))
    return truth, at, lost, datas


def host_chain(A, sym, P, Rn, word, N, h, kind, fec, level):
    """Scan, packed rows, masks, the erasure decoder (level 0: the plain one), check."""
    hits, _, _, res = F.frames(sym, P, Rn, word, 1, N)
    bits = F.bits_per_symbol(P.shape[1])
    L, B = len(word), (N * bits + 7) // 8
    before = H.rows_of(A, np.asarray(sym, np.uint8), P, hits, L, Rn, N, h, kind, fec)
    soft = X.soft_bits(P)
    after = before.copy()
    rec = np.zeros(len(hits), A.FRAME_RS_DTYPE)
    erec = np.zeros(len(hits), A.FRAME_ERASE_DTYPE)
    masks = np.zeros((len(hits), A.mask_words(B)), np.uint64)
    for i, w in enumerate(hits["window"]):
        if level:
            masks[i] = A.soft_erasures(X.row_soft(soft, len(sym), 0, int(w), L, Rn, N), level, B)
            got, r, e, _ = A.rs_frame_decode(before[i], h, kind, fec, erase=masks[i])
            erec[i] = tuple(e[f] for f in A.FRAME_ERASE_DTYPE.names)
        else:
            got, r, _ = A.rs_frame_decode(before[i], h, kind, fec)
        after[i] = got
        rec[i] = tuple(r[f] for f in A.FRAME_RS_DTYPE.names)
    chk = C.check_group(hits["window"], after, L, Rn, Z.span_of(bits, h, kind, fec), H.max_len(A, N, bits, h, kind, fec),
                        h, kind)
    return dict(hits=hits, before=before, after=after, rec=rec, erec=erec, masks=masks, chk=chk, res=res)


def test_capture_scan_producer_stage_check(A, torch, handle):
    """One graph on a side stream, replayed after the symbols and powers were
    rewritten in place: each replay's masks, rows, both records and the check's
    outputs are the host chain's for that content, and the dropout frame is
    kept."""
    d = handle(2)
    K, Rn, h, kind, fec, level = 2, 4, 1, C.CRC16, R.FLAG16, 16
    lens = (0, 60, 200, 7)
    N = Z.symbols_for(max(lens), 1, h, kind, fec) + 3
    word = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 1, 1], np.uint8)
    L = len(word)
    contents = []
    for seed, which in ((1, 1), (2, 2)):
        rng = np.random.default_rng(seed)
        truth, at, lost, datas = dropout_stream(A, K, fec, h, kind, lens, N, word, rng, which=which)
        sym, P = lay(truth, lost, K, Rn, rng)
        want = host_chain(A, sym, P, Rn, word, N, h, kind, fec, level)
        assert want["chk"][2] == datas and int(want["erec"]["used"].sum()) >= 1
        assert host_chain(A, sym, P, Rn, word, N, h, kind, fec, 0)["chk"][2] == datas[:which] + datas[which + 1:]
        contents.append((sym, P, want))
    Wn = len(contents[0][0])
    assert len(contents[1][0]) == Wn
    cap, B = 32, (N + 7) // 8
    Wm = A.mask_words(B)
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_sym, d_mag = torch.zeros(Wn, **u8), torch.zeros(Wn * K, dtype=torch.float32, device="cuda")
    d_hits, d_packed = torch.full((cap * 16,), POISONS[0], **u8), torch.full((cap * B,), POISONS[0], **u8)
    d_res, d_rs, d_erec = torch.zeros(RES_BYTES, **u8), torch.full((cap * 16,), POISONS[0], **u8), \
        torch.full((cap * 16,), POISONS[0], **u8)
    d_erase = torch.full((cap * Wm,), -1, dtype=torch.int64, device="cuda")
    d_check, d_kept = torch.full((cap * 16,), POISONS[0], **u8), torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    d_sum = torch.full((32,), POISONS[0], **u8)
    d_work = torch.zeros(A.frames_workspace_size(d.cfg, Wn), **u8)

    def enqueue(stream):
        d.frames_async(d_sym, d_mag, Wn, word, 1, N, d_hits, None, d_packed, cap, d_res, d_work, stream=stream)
        d.frames_erasures_async(d_hits, d_mag, Wn, None, d_res, 1, cap, L, N, level, d_erase, stream=stream)
        d.frames_rs_erasures_async(d_packed, d_erase, d_res, 1, cap, N, h, kind, fec, d_rs, d_erec, stream=stream)
        d.frames_check_coded_async(d_hits, d_packed, d_res, 1, cap, L, N, h, kind, d_check, d_kept, None, d_sum,
                                   fec=fec, stream=stream)

    def load(sym, P):
        d_sym.copy_(torch.from_numpy(sym))
        d_mag.copy_(torch.from_numpy(P.reshape(-1)))
        for t in (d_packed, d_rs, d_erec, d_check, d_sum):
            t.fill_(POISONS[0])
        d_erase.fill_(-1)
        torch.cuda.synchronize()

    def holds(want, what):
        torch.cuda.synchronize()
        nw = len(want["hits"])
        assert 4 <= nw <= cap, what
        rows = d_packed.cpu().numpy().reshape(cap, B)
        assert np.array_equal(rows[:nw], want["after"]) and (rows[nw:] == POISONS[0]).all(), what
        masks = d_erase.cpu().numpy().view(np.uint64).reshape(cap, Wm)
        assert np.array_equal(masks[:nw], want["masks"]) and (masks[nw:] == 2 ** 64 - 1).all(), what
        for t, w in ((d_rs, want["rec"]), (d_erec, want["erec"])):
            recs = t.cpu().numpy().reshape(cap, 16)
            assert recs[:nw].tobytes() == w.tobytes() and (recs[nw:] == POISONS[0]).all(), what
        check, kept, _, summ = want["chk"]
        assert d_check.cpu().numpy().reshape(cap, 16)[:nw].tobytes() == check.tobytes(), what
        assert d_kept.cpu().numpy().view(np.uint32)[:len(kept)].tolist() == kept.tolist(), what
        assert d_sum.cpu().numpy().view("<u8").tolist() == [summ[f] for f in ("n_checked", "n_valid", "n_kept",
                                                                              "reserved")], what

    side = torch.cuda.Stream()
    load(*contents[0][:2])
    with torch.cuda.stream(side):
        enqueue(side.cuda_stream)          # an eager call of the shape first
    holds(contents[0][2], "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for k in (1, 0, 1):
        load(*contents[k][:2])
        g.replay()
        holds(contents[k][2], ("replay", k))


# ---- 5. the one-shot call and the receiver through a dropout ----------------------------------------

_E2E = {}


def e2e_case(A):
    """Three frames at DEMOD_FEC_RS16 as 2-FSK (n 1024), data all 0xFF; the
    samples of 12 consecutive row bytes of the second frame's one codeword are 0."""
    if not _E2E:
        K, h, kind, fec, lens = 2, 1, C.CRC16, R.FLAG16, (5, 60, 7)
        rng = np.random.default_rng(12)
        word = rng.integers(0, K, 16).astype(np.uint8)
        N = Z.symbols_for(max(lens), 1, h, kind, fec) + 3
        truth, at, lost, datas = dropout_stream(A, K, fec, h, kind, lens, N, word, rng, which=1, first_byte=40)
        pcm = H.pcm_of(T.loop_tones(K), truth, 21)
        pcm[lost[0] * 1024:(lost[-1] + 1) * 1024] = 0
        _E2E.update(K=K, h=h, kind=kind, fec=fec, word=word, N=N, datas=datas, at=at, pcm=pcm, lost=lost)
    return _E2E


def test_frames_coded_through_a_dropout(A, torch, handle):
    """With DEMOD_FEC_ERASE(1) every frame comes back with its bytes; with the
    same mode without the field the dropout frame is missing and the others are
    there; both equal the host chain on the device detector's own (sym, P)."""
    c = e2e_case(A)
    d = handle(c["K"])
    K, h, kind, N, word, x, fec = c["K"], c["h"], c["kind"], c["N"], c["word"], c["pcm"], c["fec"]
    Wn = (len(x) - 1024) // 256 + 1
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_pcm = torch.from_numpy(x).cuda()
    d_sym, d_mag = torch.empty(Wn, **u8), torch.empty(Wn * K, dtype=torch.float32, device="cuda")
    d.batch_async(d_pcm, Wn, d_sym, d_mag)
    torch.cuda.synchronize()
    sym, P = d_sym.cpu().numpy(), d_mag.cpu().numpy().reshape(Wn, K)
    assert (P[[4 * s for s in c["lost"]]] == 0).all()
    for level, datas in ((1, c["datas"]), (0, c["datas"][:1] + c["datas"][2:])):
        want = host_chain(A, sym, P, 4, word, N, h, kind, fec, level)
        check, kept, bodies, summ = want["chk"]
        summ = dict(zip(summ.dtype.names, summ.tolist()))
        assert bodies == datas
        if level:
            er = want["erec"][kept[1]]
            assert (int(er["erased"]), int(er["used"]), int(er["fallback"])) == (12, 1, 0)
            assert int(want["rec"][kept[1]]["corrected"]) == 12
        for pcm in (x, d_pcm):
            g_hits, lengths, body, g_res, summary = d.frames_coded(pcm, word, max_errors=1, frame_symbols=N,
                                                                    len_bytes=h, crc=kind,
                                                                    fec=fec | A.DEMOD_FEC_ERASE(level))
            assert body == bodies and lengths.tolist() == [len(b) for b in bodies]
            assert g_hits.tobytes() == want["hits"][kept].tobytes() and summary == summ
            assert g_res["n_written"] == want["res"]["n_written"] == len(want["hits"])


def test_rx_push_through_a_dropout(A, torch, handle):
    """demod_rx_push with DEMOD_FEC_ERASE(1), three streams at three delays in
    ragged packets that split the dropout: each stream's frames are
    demod_frames_coded's on its recording, every frame; without the field the
    dropout frame is missing."""
    c = e2e_case(A)
    d = handle(c["K"])
    K, h, kind, N, word, x, fec = c["K"], c["h"], c["kind"], c["N"], c["word"], c["pcm"], c["fec"]
    rng = np.random.default_rng(3)
    recs = [x] + [np.concatenate([rng.integers(-300, 301, lead).astype(np.int16), x]) for lead in (100, 777)]
    sizes = (48000, 30011, 52345)
    assert len(c["lost"]) * 1024 > max(sizes)          # the dropout straddles a push in every stream
    for level, datas in ((1, c["datas"]), (0, c["datas"][:1] + c["datas"][2:])):
        mode = fec | A.DEMOD_FEC_ERASE(level)
        want = []
        for r in recs:
            g_hits, _, body, _, _ = d.frames_coded(r, word, max_errors=1, frame_symbols=N, len_bytes=h, crc=kind,
                                                   fec=mode)
            want.append([(int(hh["window"]), int(hh["errors"]), b) for hh, b in zip(g_hits, body)])
            assert [b for _, _, b in want[-1]] == datas
        ring = (len(recs[2]) - 1024) // 256 + 1 + 64
        rxcfg = A.make_rx_cfg(word, 1, N, h, kind, mode, 8, ring)
        got = [[] for _ in recs]
        at = [0] * len(recs)
        with A.Receiver(len(recs), rxcfg, n=1024, hop=256, freqs=T.loop_tones(K)) as rx:
            assert rx.sizes["max_len"] == H.max_len(A, N, 1, h, kind, fec)
            turn = 0
            while any(a < len(r) for a, r in zip(at, recs)):
                packets = []
                for s, r in enumerate(recs):
                    size = sizes[(turn + s) % len(sizes)]
                    packets.append(r[at[s]:at[s] + size] if at[s] < len(r) else None)
                    at[s] += size
                turn += 1
                fr, bodies, summ = rx.push(packets)
                assert summ["n_frames"] == len(fr)
                for f, b in zip(fr, bodies):
                    got[int(f["stream"])].append((int(f["window"]), int(f["errors"]), b))
        assert got == want, level


def test_widest_rows_through_the_one_shot_call_and_the_receiver(A, torch):
    """DEMOD_FEC_RS32 | DEMOD_FEC_ERASE(1) with rows of n' = 4710 bytes (h 2,
    CRC-32, 4096 data bytes, D = 19), wider than any fec-0 row: a dropout over
    40 consecutive row bytes. demod_frames_coded equals the host chain on the
    device detector's own (sym, P), and demod_rx_push gives the same frame."""
    K, h, kind, fec, n = 2, 2, C.CRC32, R.FLAG32, 256
    mode = fec | A.DEMOD_FEC_ERASE(1)
    rng = np.random.default_rng(32)
    word = rng.integers(0, K, 16).astype(np.uint8)
    N = 8 * 4710
    assert Z.symbols_for(4096, 1, h, kind, fec) == N
    truth, at, lost, datas = dropout_stream(A, K, fec, h, kind, (4096,), N, word, rng, which=0, first_byte=100,
                                            n_bytes=40)
    x = H.pcm_of(T.loop_tones(K), truth, 5, n=n)
    x[lost[0] * n:(lost[-1] + 1) * n] = 0
    Wn = len(x) // n
    u8 = dict(dtype=torch.uint8, device="cuda")
    with A.Demodulator(n=n, hop=n, freqs=T.loop_tones(K)) as d:
        d_pcm = torch.from_numpy(x).cuda()
        d_sym, d_mag = torch.empty(Wn, **u8), torch.empty(Wn * K, dtype=torch.float32, device="cuda")
        d.batch_async(d_pcm, Wn, d_sym, d_mag)
        torch.cuda.synchronize()
        sym, P = d_sym.cpu().numpy(), d_mag.cpu().numpy().reshape(Wn, K)
        want = host_chain(A, sym, P, 1, word, N, h, kind, fec, 1)
        check, kept, bodies, summ = want["chk"]
        summ = dict(zip(summ.dtype.names, summ.tolist()))
        assert bodies == datas and len(kept) == 1
        er = want["erec"][kept[0]]
        assert int(er["erased"]) == 40 and int(er["used"]) >= 19 - 1 and want["masks"].shape[1] == 74
        g_hits, lengths, body, g_res, summary = d.frames_coded(x, word, max_errors=1, frame_symbols=N, len_bytes=h,
                                                                crc=kind, fec=mode)
        assert body == bodies and g_hits.tobytes() == want["hits"][kept].tobytes() and summary == summ
    rxcfg = A.make_rx_cfg(word, 1, N, h, kind, mode, 2, 2 * (16 + N) + 64)
    got = []
    with A.Receiver(1, rxcfg, n=n, hop=n, freqs=T.loop_tones(K)) as rx:
        assert rx.sizes["row_bytes"] == 4710 and rx.sizes["max_len"] == 4096
        for a in range(0, len(x), 3000007):
            fr, bod, _ = rx.push([x[a:a + 3000007]])
            got += [(int(f["window"]), int(f["errors"]), b) for f, b in zip(fr, bod)]
    assert got == [(int(g_hits["window"][0]), int(g_hits["errors"][0]), datas[0])]


# ---- 6. refusals -------------------------------------------------------------------------------------

def test_refusals(A, torch, handle):
    """DEMOD_BAD_ARG before any launch, the outputs stay poison: the producer's
    level, K, pointers and alignment; the stage's mode, pointers and alignment;
    the field at every device entry that must keep refusing it. The one-shot
    call and the receiver take it with a parity flag alone, as the host says."""
    lib = A.load_library()
    d = handle(2)
    S, cap, N, L, Wn = 3, 4, 1024, 8, 5000
    rows = S * cap
    u8 = dict(dtype=torch.uint8, device="cuda")

    def poison(nbytes):
        return torch.full((nbytes,), POISONS[0], **u8)
    d_hits, d_res = torch.zeros(rows * 16, **u8), torch.zeros(S * RES_BYTES, **u8)
    d_mag = torch.ones(Wn * 2, dtype=torch.float32, device="cuda")
    d_rows, d_rs, d_erec, d_erase = poison(rows * 128), poison(rows * 16 + 4), poison(rows * 16 + 4), poison(rows * 16 + 8)
    d_check, d_kept, d_body, d_sum = poison(rows * 16), poison(rows * 4), poison(rows * 128), poison(S * 32)
    d_first = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    ph, pm, pr, po, prs, per, pe, pf = (t.data_ptr() for t in (d_hits, d_mag, d_res, d_rows, d_rs, d_erec, d_erase,
                                                               d_first))
    kind = A.DEMOD_CRC16_CCITT_FALSE
    lv = A.DEMOD_FEC_ERASE(16)

    def producer(level=16, h=d._h, hits=ph, mag=pm, res=pr, erase=pe, first=None, n=N, wn=Wn):
        return lib.demod_frames_erasures_async(h, hits, mag, wn, first, res, S, cap, L, n, level, erase, None)

    def stage(fec=0x100, h=d._h, rws=po, erase=pe, rs=prs, erec=per, n=N):
        return lib.demod_frames_rs_erasures_async(h, rws, erase, pr, S, cap, n, 1, kind, fec, rs, erec, None)
    bad = A.DEMOD_BAD_ARG
    assert [producer(level=v) for v in (0, -1, 128)] == [bad] * 3
    assert [producer(h=None), producer(hits=None), producer(mag=None), producer(res=None), producer(erase=None)] == [bad] * 5
    assert [producer(erase=pe + 4), producer(first=pf + 4), producer(hits=ph + 4), producer(n=0),
            producer(wn=2 ** 31), producer(n=8 * 4710 + 1)] == [bad] * 6
    with A.Demodulator(n=1024, hop=256, freqs=list(T.loop_tones(4))[:3]) as d3:   # K = 3
        assert producer(h=d3._h) == bad
    for fec in (0, 1, 0x41, 0x300, 0x100 | lv, 0x200 | lv, 0x101 | lv, 0x400):
        assert stage(fec=fec) == bad, hex(fec)
    assert [stage(h=None), stage(rws=None), stage(erase=None), stage(rs=None), stage(erec=None)] == [bad] * 5
    assert [stage(erase=pe + 4), stage(rs=prs + 2), stage(erec=per + 2), stage(n=8 * 18)] == [bad] * 4
    # the field at the entries that keep refusing it
    fec = 0x100 | lv
    assert lib.demod_frames_rs_async(d._h, po, pr, S, cap, N, 1, kind, fec, prs, None) == bad
    assert lib.demod_frames_check_coded_async(d._h, ph, po, pr, S, cap, L, N, 1, kind, fec, d_check.data_ptr(),
                                              d_kept.data_ptr(), d_body.data_ptr(), d_sum.data_ptr(), None) == bad
    need = A.fec_decode_workspace_size(d.cfg, S, cap, N, 0x101)
    d_work = poison(need)
    assert lib.demod_frames_decode_async(d._h, ph, pm, Wn, None, pr, S, cap, L, N, 1, kind, 0x101 | lv, po, prs,
                                         d_work.data_ptr(), need, None) == bad
    d_state, d_frames, d_bodies, d_rsum = torch.zeros(S * 40, **u8), poison(rows * 32), poison(rows * 128), poison(32)
    d_cwork = poison(A.rx_collect_workspace_size(d.cfg, S))

    def collect(mode):
        return lib.demod_rx_collect_async(d._h, d_state.data_ptr(), ph, pr, d_check.data_ptr(), d_kept.data_ptr(),
                                          d_body.data_ptr(), d_sum.data_ptr(), S, cap, L, N, 1, kind, mode,
                                          d_frames.data_ptr(), d_bodies.data_ptr(), d_rsum.data_ptr(),
                                          d_cwork.data_ptr(), d_cwork.numel(), None)
    assert collect(fec) == bad and collect(0x200 | A.DEMOD_FEC_ERASE(127)) == bad
    torch.cuda.synchronize()
    for t in (d_rows, d_rs, d_erec, d_erase, d_check, d_kept, d_body, d_sum, d_work, d_frames, d_bodies, d_rsum):
        assert bool((t == POISONS[0]).all())
    d_sum.zero_()
    assert collect(0x100) == A.DEMOD_OK          # the same call without the field runs
    torch.cuda.synchronize()
    # legal, the same calls run
    assert producer() == A.DEMOD_OK and producer(first=pf) == A.DEMOD_OK and stage() == A.DEMOD_OK
    assert stage(fec=0x201) == A.DEMOD_OK        # behind the Viterbi decode, with a reliability of the caller's
    torch.cuda.synchronize()
    word = [0, 1, 1, 0, 1]
    rx_base = dict(sync=word, max_errors=0, frame_symbols=1024, len_bytes=1, crc=C.CRC16, max_frames=4,
                   ring_windows=2 * 1029 * 4)
    tx_base = dict(sync=word, len_bytes=1, crc=C.CRC16, max_len=16, ring_symbols=8192)
    for mode in (lv, lv | 1, lv | 0x101, lv | 0x300):
        with pytest.raises(A.DemodError):
            A.Receiver(S, A.make_rx_cfg(fec=mode, **rx_base), n=1024, hop=256, freqs=T.loop_tones(2))
        with pytest.raises(A.DemodError):
            d.frames_coded(np.zeros(8192, np.int16), word, frame_symbols=1024, len_bytes=1, fec=mode)
        res, summ = A.DemodFramesResult(), A.DemodFramesCheckResult()
        hits, lens = np.zeros(4, A.FRAME_HIT_DTYPE), np.zeros(4, np.uint32)
        pcm = np.zeros(8192 + 8, np.int16)
        sync = np.array(word, np.uint8)
        at = pcm.ctypes.data + (-pcm.ctypes.data) % 16
        assert lib.demod_frames_coded(d._h, at, 16, sync.ctypes.data, 5, 0, 1024, 1, kind, mode, hits.ctypes.data,
                                      lens.ctypes.data, None, 4, ctypes.byref(res), ctypes.byref(summ)) == bad
    with pytest.raises(A.DemodError):
        A.Transmitter(S, A.make_tx_cfg(fec=fec, **tx_base), n=1024, hop=256, freqs=T.loop_tones(2))
    with A.Receiver(S, A.make_rx_cfg(fec=fec, **rx_base), n=1024, hop=256, freqs=T.loop_tones(2)) as rx:
        assert rx.sizes["max_len"] == H.max_len(A, 1024, 1, 1, C.CRC16, 0x100)
