"""The frame check (frames_check.hip) and the soft-decision decode
(frames_fec.hip) at every group count a segmented scan can hand them, up to
DEMOD_MAX_SEGMENTS, against tests/frames_check_ref.py, tests/frames_fec_ref.py
and tests/frames_segments_ref.py; and the other launches that walk their rows
the same way (the outer code's stage, the transmitter's write, the receiver's
copy) across the same cap, against the host references of their own tests.

The stages size their launch from a cap of 16384 waves a call: with most =
16384 / S (at least 1) a group gets wpg = min(max_frames, most) waves (the
body kernel min(ceil(max_frames max_len / 64), most)). The cases here reach
what the neighbouring files do not: most below max_frames, most = 1 and the
16384 / S == 0 fallback, a last block with waves that leave beside live ones,
the body kernel's stride loop running more than once, workspace slots above
16383, the decode of a punctured and interleaved mode (tests/fec_modes_ref.py),
whose workspace goes by the mode's step count, at two of these counts, and the
chain segmented scan -> decode -> coded check behind 20000
segments, nearly all of them empty.

A group's outputs depend on its own content alone (test_groups and
test_segments of the neighbouring files assert that), so the host reference is
computed once for a pool of at most 64 distinct groups (hits, rows or powers,
stored count) and laid out by the same seeded indices that fill the S groups.
As everywhere: every output is poisoned and compared WHOLE with the reference
laid over the same poison, and the inputs are compared byte for byte after the
call.

Out of scope: frames_kept_rows_kernel's grid is capped at 1024 blocks, which
matters only above 262144 kept frames in one synchronous call (its loop then
strides); no group count reaches it.
"""
import functools

import numpy as np
import pytest

import fec_modes_ref as Z
import frames_check_ref as C
import frames_fec_ref as X
import frames_ref as F
import frames_segments_ref as FS
import guards as G
import rs_ref as RS
import rx_ref as RX
import test_gpu_fec_modes as TM
import test_gpu_frames_check as TC
import test_gpu_frames_fec as TF
import test_gpu_frames_segments as TS
import test_gpu_rs as TR
import test_gpu_rx as TX
import test_gpu_tx as TT
import tx_ref as T
from gpu_support import frames_result_bytes as result_bytes, handle_fixture, phased, tones_375, torch  # noqa: F401

pytestmark = pytest.mark.gpu

MAX_WAVES = 16384            # kRowMaxWaves (csrc/frame_rows.h)
WAVES_PER_BLOCK = 4
LANES = 64
LEAD = 4096
# (S, max_frames, most, waves of the check's and the decode's launch)
GEOMETRY = [(4096, 5, 4, 16384), (5461, 4, 3, 16383), (8193, 3, 1, 8193), (16384, 2, 1, 16384),
            (16385, 3, 1, 16385), (65536, 2, 1, 65536)]
POOL = 48                    # distinct groups of a case
LIVE = {5461: 3, 8193: 1, 16385: 1}   # live waves of a partial last block (wpg = most in every launch here)


# handle(R, K): one Demodulator per (R, K), closed with the module.
handle = handle_fixture(lambda A, Rn, K: phased(A, TC.SHAPE_OF_R, Rn, tones_375(K)))


# ---- the launch arithmetic, restated from the kernels' comments ---------------------

def waves_per_group(S, max_frames):
    most = MAX_WAVES // S if MAX_WAVES // S else 1
    return min(max_frames, most)


def body_waves_per_group(S, max_frames, max_len):
    most = MAX_WAVES // S if MAX_WAVES // S else 1
    return min(-(-max_frames * max_len // LANES), most)


def last_block(S, wpg):
    """(live waves of the launch's last block, the groups they belong to)."""
    waves = S * wpg
    live = waves % WAVES_PER_BLOCK or WAVES_PER_BLOCK
    return live, sorted({w // wpg for w in range(waves - live, waves)})


def stored_counts(rng, max_frames):
    """POOL stored n_written: entry 0 max_frames, 1 zero, 2 above max_frames,
    3 2^64 - 1, the rest drawn from [0, max_frames]."""
    counts = [int(v) for v in rng.integers(0, max_frames + 1, POOL)]
    counts[:4] = [max_frames, 0, max_frames + 7, 2 ** 64 - 1]
    return counts


def draw_slots(rng, S):
    """The pool entry of each of the S groups: entry 0 (max_frames rows) in
    groups 0 and S - 1, entry 1 (no rows) in group 1."""
    idx = rng.integers(0, POOL, S)
    idx[0], idx[1], idx[S - 1] = 0, 1, 0
    assert {2, 3} <= set(idx.tolist())             # a stored count above max_frames, and 2^64 - 1
    return idx


def tally(S, max_frames, idx, counts, statuses):
    """Groups, rows, empty groups and rows per status of a case (statuses: per
    pool entry, the statuses of its rows)."""
    nw = np.array([min(c, max_frames) for c in counts])[idx]
    per = {}
    use = np.bincount(idx, minlength=POOL)
    for p, st in enumerate(statuses):
        for s in st:
            per[int(s)] = per.get(int(s), 0) + int(use[p])
    return dict(groups=S, rows=int(nw.sum()), empty=int((nw == 0).sum()), status=dict(sorted(per.items())))


def assert_last_block_holds_rows(S, wpg, idx, counts, max_frames, want_live):
    live, groups = last_block(S, wpg)
    assert live == want_live, (S, wpg, live)
    if live < WAVES_PER_BLOCK:                     # a wave leaves beside these: they must have work
        for g in groups:
            assert min(counts[idx[g]], max_frames) > 0, (S, g)


# ---- Part 1: the check ----------------------------------------------------------------

BIG = dict(Rn=1, K=16, L=24, B=65, h=2, kind=C.CRC32)           # max_len 59: the body kernel strides
SMALL = dict(Rn=4, K=2, L=TC.SELECT_L, B=TC.SELECT_B, h=TC.SELECT_H, kind=TC.SELECT_KIND)


def big_group(rng, n_rows, full, Rn, L, B, h, kind, bits):
    """n_rows rows with ascending windows and drawn roles: kept (at or past
    everything before it), covered (inside a valid frame before it), invalid (a
    flipped bit in data or CRC), random (a drawn header, random bytes) and long
    (a header of max_len + 1). full: every row a kept frame of max_len bytes."""
    c = C.CRC_BYTES[kind]
    max_len = B - h - c
    windows = np.zeros(n_rows, np.uint64)
    rows = np.zeros((n_rows, B), np.uint8)
    w, reach = int(rng.integers(0, 3)) * Rn, 0
    for i in range(n_rows):
        role = "kept" if full else ("kept", "covered", "invalid", "random", "long")[int(rng.integers(0, 5))]
        length = max_len if full or rng.integers(0, 3) == 0 else int(rng.integers(0, max_len + 1))
        w += Rn
        if role == "kept":
            w = max(w, reach) + Rn * int(rng.integers(0, 3))
        if role in ("kept", "covered"):
            rows[i] = TC.frame_row(rng, length, B, h, kind)
        elif role == "invalid":
            rows[i] = TC.flip(TC.frame_row(rng, length, B, h, kind), h, h + length + c, rng)
        else:
            rows[i] = rng.integers(0, 256, B)
            head = max_len + 1 if role == "long" else int(rng.integers(0, max_len + 3))
            rows[i, :h] = np.frombuffer(head.to_bytes(h, "big"), np.uint8)
        windows[i] = w
        got = C.check_row(rows[i], h, kind)
        if got[2] == C.OK:
            reach = max(reach, w + (L + C.frame_symbols(h + got[0] + c, bits)) * Rn)
    return windows, rows


@functools.lru_cache(maxsize=2)
def check_case(S, max_frames, small=False):
    """One case: (shape, the pool's hits [POOL][max_frames], packed rows and
    stored counts, idx: the pool entry of each of the S groups)."""
    shape = SMALL if small else BIG
    Rn, K, L, B, h, kind = (shape[k] for k in ("Rn", "K", "L", "B", "h", "kind"))
    bits = F.bits_per_symbol(K)
    rng = np.random.default_rng(S * 10 + max_frames + (1 if small else 0))
    counts = stored_counts(rng, max_frames)
    hits = np.zeros((POOL, max_frames), C.HIT_DTYPE)
    packed = np.zeros((POOL, max_frames, B), np.uint8)
    for p in range(POOL):
        if small:
            hits["window"][p], packed[p], _ = TC.select_group(rng, min(counts[p], max_frames), max_frames, Rn, bits)
        else:
            hits["window"][p], packed[p] = big_group(rng, max_frames, p == 0, Rn, L, B, h, kind, bits)
        hits["errors"][p] = rng.integers(0, 3, max_frames)
    idx = draw_slots(rng, S)
    return shape, hits, packed, counts, idx


def check_expected(case, poison=TC.POISON):
    """The four outputs of the S groups whole, from the pool's reference."""
    shape, hits, packed, counts, idx = case
    bits = F.bits_per_symbol(shape["K"])
    want, refs = TC.expected(hits, packed, counts, shape["L"], shape["Rn"], bits, shape["h"], shape["kind"], poison)
    return {k: v[idx] for k, v in want.items()}, refs


def late_bytes(refs, idx, max_len, step):
    """Body bytes at e = r max_len + b >= step: written by a second or later
    pass of the body kernel's loop alone."""
    per = [sum(len(d) - min(max(step - r * max_len, 0), len(d)) for r, d in enumerate(ref[2])) for ref in refs]
    return int(np.array(per)[idx].sum())


def run_check(torch, d, case, hits, packed, counts, body=True, poison=TC.POISON, guard=False):
    shape = case[0]
    N = TC.row_symbols(shape["B"], F.bits_per_symbol(shape["K"]))
    return TC.Run(torch, hits, packed, counts, body=body, poison=poison, guard=guard)(
        d, shape["L"], N, shape["h"], shape["kind"])


def check_fixture(case, refs, S, max_frames, most, waves):
    """The fixture's conditions, on the reference alone. Returns the tally."""
    shape, hits, packed, counts, idx = case
    max_len = shape["B"] - shape["h"] - C.CRC_BYTES[shape["kind"]]
    wpg = waves_per_group(S, max_frames)
    assert (MAX_WAVES // S if MAX_WAVES // S else 1) == most and S * wpg == waves
    assert_last_block_holds_rows(S, wpg, idx, counts, max_frames, LIVE.get(S, WAVES_PER_BLOCK))
    status = np.concatenate([r[0]["status"] for r in refs])
    covered = np.concatenate([r[0]["covered"] for r in refs])
    assert set(status.tolist()) == {C.OK, C.BAD_LENGTH, C.BAD_CRC}
    assert covered.sum() > 0 and sum(len(r[1]) for r in refs) > 0
    stats = tally(S, max_frames, idx, counts, [r[0]["status"] for r in refs])
    if shape is BIG:
        bwpg = body_waves_per_group(S, max_frames, max_len)
        assert max_frames * max_len > LANES * most and bwpg == most          # the loop strides
        assert_last_block_holds_rows(S, bwpg, idx, counts, max_frames, LIVE.get(S, WAVES_PER_BLOCK))
        chk, kept, bodies, summ = refs[0]                                    # groups 0 and S - 1
        assert summ["n_kept"] == max_frames and len(bodies[-1]) == max_len
        stats["late_bytes"] = late_bytes(refs, idx, max_len, bwpg * LANES)
        assert stats["late_bytes"] > 0
    return stats


@pytest.mark.parametrize("S,max_frames,most,waves", GEOMETRY)
def test_check_geometry(A, torch, handle, S, max_frames, most, waves):
    """h 2, CRC-32, rows of 65 bytes (max_len 59) at every (S, max_frames) of
    the table: the check, the selection and the body, whose loop strides. At
    S = 16385 also the same content rotated by one slot: each group's bytes move
    with it."""
    case = check_case(S, max_frames)
    shape, hits, packed, counts, idx = case
    want, refs = check_expected(case)
    stats = check_fixture(case, refs, S, max_frames, most, waves)
    print(f"check S={S} max_frames={max_frames}: {stats}")
    d = handle(shape["Rn"], shape["K"])
    full = [counts[p] for p in idx]
    got = run_check(torch, d, case, hits[idx], packed[idx], full)
    TC.same(got, want, S)
    if S == 16385:
        order = np.roll(np.arange(S), -1)                     # slot g holds group g + 1's content
        got2 = run_check(torch, d, case, hits[idx[order]], packed[idx[order]], [full[g] for g in order])
        TC.same(got2, {k: v[order] for k, v in want.items()}, "rotated")
        for k in got:
            assert np.array_equal(got2[k], got[k][order]), k


@pytest.mark.parametrize("small,body,guard", [(False, False, False), (True, True, True)])
def test_check_fallback_shapes(A, torch, handle, small, body, guard):
    """S = 16385 x 3 rows again: without d_body, and in the CRC-16, h 1, 8-byte
    shape of test_select_shapes between poisoned guards with two poisons."""
    S, max_frames, most, waves = GEOMETRY[4]
    case = check_case(S, max_frames, small)
    shape, hits, packed, counts, idx = case
    d = handle(shape["Rn"], shape["K"])
    full = [counts[p] for p in idx]
    for poison in (0xFF, 0x5A) if guard else (0xFF,):
        want, refs = check_expected(case, poison)
        stats = check_fixture(case, refs, S, max_frames, most, waves)
        got = run_check(torch, d, case, hits[idx], packed[idx], full, body=body, poison=poison, guard=guard)
        assert ("body" in got) == body
        TC.same(got, want, poison)
    print(f"check S={S} max_frames={max_frames} small={small} body={body}: {stats}")


# ---- Part 1: the decode ------------------------------------------------------------------

def decode_rows_pool(rng, K, Rn, h, kind, N, count=40):
    """`count` rows of one shape laid in one batch: frames of drawn lengths (0,
    1 and max_len among them) with 4 flipped coded bits each, every fourth a
    random row, one a header of max_len + 1. Returns (P, starts, frames: the
    planted frame of each row, or None)."""
    bits = F.bits_per_symbol(K)
    St, Bd, max_len = X.row_shape(N, bits, h, kind)
    rows, frames = [], []
    for r in range(count):
        if r % 4 == 3:
            rows.append(rng.integers(0, K, N).astype(np.uint8))
            frames.append(None)
        elif r == 5:
            info = (max_len + 1).to_bytes(h, "big") + rng.integers(0, 256, Bd).astype(np.uint8).tobytes()
            rows.append(TF.info_symbols(info, St, N, bits, rng, 0))
            frames.append(None)
        else:
            length = (0, 1, max_len)[r] if r < 3 else int(rng.integers(0, max_len + 1))
            row, frame = TF.frame_symbols(rng, length, N, bits, h, kind)
            rows.append(row)
            frames.append(frame)
    P, starts = TF.lay_rows(rows, K, Rn, rng)
    return P, starts, frames


@functools.lru_cache(maxsize=2)
def decode_case(S, max_frames, K, Rn, tables):
    """One case's inputs with its pool: h 1, CRC-16, the minimal N. tables: the
    groups carry a first[] entry of 0, `shift` (the same rows, their windows
    relative), n_windows - a few symbols (the row's end erased), n_windows and
    two above it."""
    h, kind = 1, C.CRC16
    bits = F.bits_per_symbol(K)
    N = TF.min_symbols(bits, h)
    assert X.row_shape(N, bits, h, kind) == (72, 8, 5)
    rng = np.random.default_rng(S * 10 + max_frames + K)
    P, starts, frames = decode_rows_pool(rng, K, Rn, h, kind, N)
    W = len(P)
    counts = stored_counts(rng, max_frames)
    hits = np.zeros((POOL, max_frames), C.HIT_DTYPE)
    hits["window"] = starts[rng.integers(0, len(starts), hits.shape)]
    hits["errors"] = rng.integers(0, 3, hits.shape)
    first = None
    shift = int(starts[3])
    if tables:
        choices = [0, shift, W - (TF.L0 + 20) * Rn, 0, W, shift, W + 9, 2 ** 64 - 1]
        first = [choices[p % len(choices)] for p in range(POOL)]
        for p, f in enumerate(first):
            if f == shift:
                hits["window"][p] = starts[rng.integers(3, len(starts), max_frames)] - np.uint64(shift)
            elif f:
                hits["window"][p] = rng.integers(0, 3 * Rn + 1, max_frames).astype(np.uint64)
    idx = draw_slots(rng, S)
    planted = {int(s): f for s, f in zip(starts, frames) if f is not None}
    return dict(K=K, Rn=Rn, h=h, kind=kind, N=N, P=P, W=W, hits=hits, counts=counts, first=first, idx=idx,
                planted=planted, bases=(0, shift) if tables else (0,))


def decode_expected(case, S, max_frames, most, waves, poison=TF.POISON):
    """rows and decode of the S groups whole, from the pool's reference; the
    fixture's conditions on the reference alone; the tally."""
    c = case
    rows, dec, by_key = TF.reference(c["P"], c["W"], c["first"], c["hits"], c["counts"], TF.L0, c["Rn"], c["N"],
                                     c["h"], c["kind"], poison)
    idx = c["idx"]
    wpg = waves_per_group(S, max_frames)
    assert (MAX_WAVES // S if MAX_WAVES // S else 1) == most and S * wpg == waves
    assert_last_block_holds_rows(S, wpg, idx, c["counts"], max_frames, LIVE.get(S, WAVES_PER_BLOCK))
    back = 0
    for key, (written, d) in by_key.items():
        base, w = key if key is not None else (None, 0)
        frame = c["planted"].get(base + w) if base in c["bases"] else None
        if frame is not None:
            assert written == frame and d["status"] == X.OK, (base, w)
            back += 1
    assert back >= 10
    assert {int(v[1]["status"]) for v in by_key.values()} == {X.OK, X.BAD_LENGTH}
    statuses = [dec[p, :min(c["counts"][p], max_frames)].copy().view(X.DECODE_DTYPE)["status"].reshape(-1)
                for p in range(POOL)]
    return (rows[idx], dec[idx]), tally(S, max_frames, idx, c["counts"], statuses)


def run_decode(A, torch, d, case, idx, **kw):
    c = case
    first = None if c["first"] is None else [c["first"][p] for p in idx]
    return TF.Run(A, torch, c["P"], c["hits"][idx], [c["counts"][p] for p in idx], first=first, **kw)(
        d, TF.L0, c["N"], c["h"], c["kind"])


@pytest.mark.parametrize("S,max_frames,most,waves", GEOMETRY)
def test_decode_geometry(A, torch, handle, S, max_frames, most, waves):
    """16 tones, R 1, h 1, CRC-16, the minimal rows (72 steps, 8 bytes) at
    every (S, max_frames) of the table; the workspace (S wpg slots of 72 words:
    37748736 bytes at S = 65536) under two poisons. At S = 16385 also the same
    content rotated by one slot."""
    K, Rn = 16, 1
    case = decode_case(S, max_frames, K, Rn, False)
    want, stats = decode_expected(case, S, max_frames, most, waves)
    print(f"decode S={S} max_frames={max_frames}: {stats}")
    d = handle(Rn, K)
    need = A.frames_decode_workspace_size(d.cfg, S, max_frames, case["N"])
    assert need == waves * 72 * 8 and (S != 65536 or need == 65536 * 72 * 8)
    idx = case["idx"]
    for work_poison in (0xFF, 0x00):
        got = run_decode(A, torch, d, case, idx, work_poison=work_poison)
        TF.same(got, want, (S, work_poison))
    if S == 16385:
        order = np.roll(np.arange(S), -1)                     # slot g holds group g + 1's content
        got2 = run_decode(A, torch, d, case, idx[order])
        TF.same(got2, [v[order] for v in want], "rotated")
        for a, b in zip(got2, got):
            assert np.array_equal(a, b[order])


def test_decode_fallback_tables(A, torch, handle):
    """S = 16385 x 3 rows again at 2 tones, R 4, with a first[] table (entries
    at n_windows and above it among them), between poisoned guards with two
    poisons."""
    S, max_frames, most, waves = GEOMETRY[4]
    K, Rn = 2, 4
    case = decode_case(S, max_frames, K, Rn, True)
    assert case["W"] in case["first"] and max(case["first"]) > case["W"]
    d = handle(Rn, K)
    for poison in (0xFF, 0x5A):
        want, stats = decode_expected(case, S, max_frames, most, waves, poison)
        got = run_decode(A, torch, d, case, case["idx"], poison=poison, guard=True)
        TF.same(got, want, poison)
    print(f"decode S={S} max_frames={max_frames} K={K} R={Rn} with first[]: {stats}")


# ---- Part 2: the mapped decode (fec_modes_ref) at the same group counts ---------------------------

@functools.lru_cache(maxsize=2)
def mapped_decode_case(S, max_frames, fec, Rn, tables):
    """decode_case in a mapped mode at 2 tones: h 1, CRC-16, rows of one
    interleaver block (N = 256 symbols at 1 bit, the least the mode accepts),
    a pool of 40 rows (test_gpu_fec_modes.pool) and POOL distinct groups."""
    K, h, kind, N = 2, 1, C.CRC16, Z.BLOCK
    assert Z.row_shape(N, 1, h, kind, fec) is not None and Z.row_shape(N - 1, 1, h, kind, fec) is None
    rng = np.random.default_rng(S * 10 + max_frames + fec)
    P, starts = TM.pool(rng, K, Rn, h, kind, fec, N, 40)
    W = len(P)
    counts = stored_counts(rng, max_frames)
    hits = np.zeros((POOL, max_frames), C.HIT_DTYPE)
    hits["window"] = starts[rng.integers(0, len(starts), hits.shape)]
    hits["errors"] = rng.integers(0, 3, hits.shape)
    first = None
    if tables:
        shift = int(starts[3])
        choices = [0, shift, W - (TM.L0 + 20) * Rn, 0, W, shift, W + 9, 2 ** 64 - 1]
        first = [choices[p % len(choices)] for p in range(POOL)]
        for p, f in enumerate(first):
            if f == shift:
                hits["window"][p] = starts[rng.integers(3, len(starts), max_frames)] - np.uint64(shift)
            elif f:
                hits["window"][p] = rng.integers(0, 3 * Rn + 1, max_frames).astype(np.uint64)
    return dict(K=K, Rn=Rn, h=h, kind=kind, N=N, fec=fec, P=P, W=W, hits=hits, counts=counts, first=first,
                idx=draw_slots(rng, S))


def mapped_decode_expected(A, case, S, max_frames, most, waves, poison=TM.POISON):
    """rows and decode of the S groups whole, from the pool's reference (the
    host decoder on the reference's soft values, which tests/test_fec_modes_cpu.py
    holds to fec_modes_ref.decode); the fixture's conditions; the tally."""
    c = case
    rows, dec, by_key = TM.reference(A, c["P"], c["W"], c["first"], c["hits"], c["counts"], TM.L0, c["Rn"], c["N"],
                                     c["h"], c["kind"], c["fec"], poison)
    idx = c["idx"]
    wpg = waves_per_group(S, max_frames)
    assert (MAX_WAVES // S if MAX_WAVES // S else 1) == most and S * wpg == waves
    assert_last_block_holds_rows(S, wpg, idx, c["counts"], max_frames, LIVE.get(S, WAVES_PER_BLOCK))
    assert {int(v[1]["status"][0]) for v in by_key.values()} == {X.OK, X.BAD_LENGTH}
    assert len(by_key) >= 20                              # distinct rows decoded: a handful, not S max_frames
    statuses = [dec[p, :min(c["counts"][p], max_frames)].copy().view(X.DECODE_DTYPE)["status"].reshape(-1)
                for p in range(POOL)]
    return (rows[idx], dec[idx]), tally(S, max_frames, idx, c["counts"], statuses)


def run_mapped_decode(A, torch, d, case, idx, **kw):
    """One call; the workspace has exactly demod_fec_decode_workspace_size bytes."""
    c = case
    first = None if c["first"] is None else [c["first"][p] for p in idx]
    run = TM.Run(A, torch, c["P"], c["hits"][idx], [c["counts"][p] for p in idx], first=first, **kw)
    got = run(d, TM.L0, c["N"], c["h"], c["kind"], c["fec"])
    St = Z.row_shape(c["N"], 1, c["h"], c["kind"], c["fec"])[0]
    assert run.d_work.numel() == len(idx) * waves_per_group(len(idx), c["hits"].shape[1]) * St * 8
    return got


def test_decode_geometry_mapped(A, torch, handle):
    """Mode 0x61 (rate 3/4, interleaved: 192 steps, 23 bytes a row) at S = 5461
    x 4 rows: 3 waves a group take 4 rows, the last block has a wave that
    leaves; the workspace under two poisons."""
    S, max_frames, most, waves = GEOMETRY[1]
    fec, Rn = 0x61, 1
    assert Z.row_shape(Z.BLOCK, 1, 1, C.CRC16, fec) == (192, 23, 20)
    case = mapped_decode_case(S, max_frames, fec, Rn, False)
    want, stats = mapped_decode_expected(A, case, S, max_frames, most, waves)
    print(f"decode fec={fec:#x} S={S} max_frames={max_frames}: {stats}")
    d = handle(Rn, case["K"])
    for work_poison in (0xFF, 0x00):
        TM.same(run_mapped_decode(A, torch, d, case, case["idx"], work_poison=work_poison), want, (S, work_poison))


def test_decode_fallback_mapped(A, torch, handle):
    """Mode 0x51 (rate 2/3, interleaved: 170 steps, 20 bytes a row) at S =
    16385 x 3 rows, 2 tones, R 4, with a first[] table (entries at n_windows
    and above it among them): one wave a group, workspace slots above 16383;
    two output poisons, two workspace poisons."""
    S, max_frames, most, waves = GEOMETRY[4]
    fec, Rn = 0x51, 4
    assert Z.row_shape(Z.BLOCK, 1, 1, C.CRC16, fec) == (170, 20, 17)
    case = mapped_decode_case(S, max_frames, fec, Rn, True)
    assert case["W"] in case["first"] and max(case["first"]) > case["W"]
    d = handle(Rn, case["K"])
    for poison, work_poison in ((0xFF, 0x00), (0x5A, 0xFF)):
        want, stats = mapped_decode_expected(A, case, S, max_frames, most, waves, poison)
        got = run_mapped_decode(A, torch, d, case, case["idx"], poison=poison, work_poison=work_poison)
        TM.same(got, want, (poison, work_poison))
    print(f"decode fec={fec:#x} S={S} max_frames={max_frames} R={Rn} with first[]: {stats}")


# ---- Part 3: the chain behind a sparse segmented scan -----------------------------------------

CH = dict(S=20000, Rn=1, K=16, L=8, h=1, kind=C.CRC16, cap=2, planted=64, short=300)
CH_N = Z.symbols_for(6, 4, CH["h"], CH["kind"], X.CONV_K7)
CH_ST, CH_BD, CH_MAX = X.row_shape(CH_N, 4, CH["h"], CH["kind"])


@functools.lru_cache(maxsize=1)
def chain_content():
    """sym[Wb], P[Wb][16], the word, first[], count[] and what was planted: 64
    of the 20000 segments (the last among them) hold one coded frame each, from
    a pool of 16, with three payload symbols on a wrong tone; 300 are shorter
    than L + N windows (every third starts with the word: a tail, no frame);
    the rest have count 0."""
    S, K, L, h, kind, N = CH["S"], CH["K"], CH["L"], CH["h"], CH["kind"], CH_N
    rng = np.random.default_rng(S)
    word = np.array([3, 14, 1, 5, 9, 2, 6, 11], np.uint8)
    picks = rng.choice(S - 1, CH["planted"] - 1 + CH["short"], replace=False)
    planted = np.sort(np.r_[picks[:CH["planted"] - 1], S - 1])
    short = np.sort(picks[CH["planted"] - 1:])
    assert (planted > 16384).sum() >= 3 and planted[-1] == S - 1
    lead = {int(s): int(rng.integers(0, 6)) for s in planted}
    count = np.zeros(S, np.int64)
    for s in planted:
        count[s] = lead[int(s)] + L + N + int(rng.integers(0, 7))
    count[short] = rng.integers(1, L + N, len(short))
    first = np.cumsum(count + rng.integers(0, 3, S)) - count
    Wb = int(first[-1] + count[-1]) + 3
    sym = rng.integers(0, K, Wb).astype(np.uint8)
    lengths = [0, 1, 6, 6] + [int(v) for v in rng.integers(0, 7, 12)]
    frames = [TF.frame_symbols(rng, n, N, 4, h, kind, flips=0) for n in lengths]
    datas = {}
    for s in planted:
        row, frame = frames[int(rng.integers(0, len(frames)))]
        row = row.copy()
        Sc = X.coded_symbols(len(frame) - h - 2, h, kind, 4)
        for j in (Sc // 6, Sc // 2, (5 * Sc) // 6):
            row[j] = (row[j] + 1 + int(rng.integers(0, K - 1))) % K
        w = int(first[s]) + lead[int(s)]
        sym[w:w + L] = word
        sym[w + L:w + L + N] = row
        datas[int(s)] = (lead[int(s)], frame[h:len(frame) - 2])
    for s in short[::3]:
        if count[s] >= L:
            sym[first[s]:first[s] + L] = word
    P = TF.powers_for(sym, K, rng)
    return sym, P, word, first, count, planted, short, datas


@functools.lru_cache(maxsize=1)
def chain_reference(A):
    """Every output of the three calls whole over 0xFF, and the fixture's
    conditions on the reference alone."""
    sym, P, word, first, count, planted, short, datas = chain_content()
    S, Rn, L, h, kind, cap, N = CH["S"], CH["Rn"], CH["L"], CH["h"], CH["kind"], CH["cap"], CH_N
    B = (N * 4 + 7) // 8
    Wb = len(sym)
    want = dict(hits=np.full((S, cap, TS.HIT), 0xFF, np.uint8), payload=np.full((S, cap, N), 0xFF, np.uint8),
                packed=np.full((S, cap, B), 0xFF, np.uint8))
    # segments without windows: the closed form of a short segment (test_max_segments checks its
    # all-hit cousin the same way), held to the reference on a sample below
    empty = np.zeros((), F.RESULT_DTYPE)
    empty["phases"], empty["tail_window"] = Rn, -1
    res = np.tile(np.frombuffer(empty.tobytes(), np.uint8), (S, 1))
    some = np.flatnonzero(count > 0)
    assert len(some) == CH["planted"] + CH["short"]
    h2 = np.zeros((S, cap), C.HIT_DTYPE)
    n_written = np.zeros(S, np.int64)
    tails = 0
    for s, (r_hits, r_pay, r_pak, r_res) in zip(some, FS.frames_segments(sym, P, Rn, first[some], count[some], word,
                                                                         0, N, max_frames=cap)):
        nw = r_res["n_written"]
        res[s] = np.frombuffer(result_bytes(A, r_res), np.uint8)
        want["hits"][s, :nw] = r_hits.view(np.uint8).reshape(nw, TS.HIT)
        want["payload"][s, :nw], want["packed"][s, :nw] = r_pay, r_pak
        h2[s, :nw], n_written[s] = r_hits, nw
        tails += r_res["tail_window"] >= 0
    assert tails >= 50
    none = np.flatnonzero(count == 0)
    pick = none[::397]
    for s, r in zip(pick, FS.frames_segments(sym, P, Rn, first[pick], count[pick], word, 0, N, max_frames=cap)):
        assert result_bytes(A, r[3]) == empty.tobytes() and len(r[0]) == 0, s
    want["results"] = res
    rows, dec, _ = TF.reference(P, Wb, first, h2, n_written, L, Rn, N, h, kind)
    chk, refs = TF.coded_expected(h2, rows, n_written, L, Rn, 4, h, kind)
    want.update(rows=rows, decode=dec, **chk)
    # the fixture's conditions: every planted frame is kept, with its exact bytes
    for s in planted:
        at, data = datas[int(s)]
        kept = [int(h2[s, i]["window"]) for i in refs[s][1]]
        assert at in kept and refs[s][2][kept.index(at)] == data, s
    extra = sum(len(r[1]) for r in refs) - len(planted)
    assert extra == 0            # counted on the reference: the filler of this seed holds no frame of its own
    stats = dict(groups=S, rows=int(n_written.sum()), empty=int((n_written == 0).sum()),
                 no_windows=len(none), kept=sum(len(r[1]) for r in refs),
                 status={int(k): int(v) for k, v in zip(*np.unique(
                     np.concatenate([r[0]["status"] for r in refs]), return_counts=True))})
    return want, stats


class Chain:
    """The three calls' device buffers, every output and workspace between
    poisoned guards."""

    SCAN = ("hits", "payload", "packed", "results")
    LATER = ("rows", "decode", "check", "kept", "body", "summary")

    def __init__(self, A, torch, d):
        self.A, self.torch, self.d = A, torch, d
        sym, P, word, first, count = chain_content()[:5]
        S, cap, N = CH["S"], CH["cap"], CH_N
        self.word, self.Wb = word, len(sym)
        self.inputs = [sym, np.ascontiguousarray(P).reshape(-1), np.ascontiguousarray(first, np.uint64).view(np.int64),
                       np.ascontiguousarray(count, np.uint32).view(np.int32)]
        self.d_in = [torch.from_numpy(a.copy()).cuda() for a in self.inputs]
        rows = S * cap
        sizes = dict(hits=rows * TS.HIT, payload=rows * N, packed=rows * ((N * 4 + 7) // 8),
                     results=S * TS.RES_BYTES, rows=rows * CH_BD, decode=rows * 16, check=rows * 16,
                     kept=rows * 4, body=rows * CH_MAX, summary=S * 32,
                     work=A.frames_segments_workspace_size(d.cfg, S, self.Wb),
                     fwork=A.frames_decode_workspace_size(d.cfg, S, cap, N))
        assert sizes["fwork"] == S * CH_ST * 8
        self.shape = dict(hits=(S, cap, TS.HIT), payload=(S, cap, N), packed=(S, cap, (N * 4 + 7) // 8),
                          results=(S, TS.RES_BYTES), rows=(S, cap, CH_BD), decode=(S, cap, 16), check=(S, cap, 16),
                          kept=(S, cap, 4), body=(S, cap, CH_MAX), summary=(S, 32))
        self.t, self.guards = {}, []
        for k, nbytes in sizes.items():
            self.t[k], chk = G.guarded(torch, nbytes, torch.uint8, LEAD, LEAD, 0xFF)
            self.guards.append(chk)

    def poison(self, names):
        for k in names:
            self.t[k].fill_(0xFF)

    def scan(self, stream=0):
        t, i = self.t, self.d_in
        self.d.frames_segments_async(i[0], i[1], self.Wb, i[2], i[3], CH["S"], self.word, 0, CH_N, t["hits"],
                                     t["payload"], t["packed"], CH["cap"], t["results"], t["work"], stream=stream)

    def later(self, stream=0):
        t, i, c = self.t, self.d_in, CH
        self.d.frames_decode_async(t["hits"], i[1], self.Wb, i[2], t["results"], c["S"], c["cap"], c["L"], CH_N,
                                   c["h"], c["kind"], t["rows"], t["decode"], t["fwork"], stream=stream)
        self.d.frames_check_coded_async(t["hits"], t["rows"], t["results"], c["S"], c["cap"], c["L"], CH_N, c["h"],
                                        c["kind"], t["check"], t["kept"].view(self.torch.int32), t["body"],
                                        t["summary"], stream=stream)

    def results(self, names):
        self.torch.cuda.synchronize()
        for chk in self.guards:
            chk(written=False)
        for t, a in zip(self.d_in, self.inputs):
            assert t.cpu().numpy().tobytes() == a.tobytes(), "an input was written to"
        return {k: self.t[k].cpu().numpy().reshape(self.shape[k]) for k in names}


def test_chain_behind_sparse_scan(A, torch, handle):
    """demod_frames_segments_async -> demod_frames_decode_async (the scan's
    d_first) -> demod_frames_check_coded_async with a body on 20000 segments,
    19636 of them without a window: every output of the three calls is the
    reference's, whole; all 64 planted frames are kept although three payload
    symbols of each sit on a wrong tone. Then the last two calls captured on a
    side stream and replayed once over poisoned outputs."""
    want, stats = chain_reference(A)
    print(f"chain: {stats}")
    ch = Chain(A, torch, handle(CH["Rn"], CH["K"]))
    ch.scan()
    ch.later()
    TF.same(ch.results(Chain.SCAN + Chain.LATER), want, "eager")
    side = torch.cuda.Stream()
    ch.poison(Chain.LATER + ("fwork",))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ch.later(stream=side.cuda_stream)                 # an eager call of the shape on the stream first
        side.synchronize()
    TF.same(ch.results(Chain.LATER), want, "side stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ch.later(stream=torch.cuda.current_stream().cuda_stream)
    ch.poison(Chain.LATER + ("fwork",))
    torch.cuda.synchronize()
    g.replay()
    TF.same(ch.results(Chain.SCAN + Chain.LATER), want, "replay")


# ---- Part 4: the other launches on the same walk (csrc/frame_rows.h) -----------------------------

RS_FLAG, RS_H, RS_KIND = RS.FLAG16, 1, C.CRC16


def rs_width():
    """The shortest row that holds two codewords at parity 16: n = 240 bytes
    (239 fill one codeword), n' = 272."""
    P = RS.PARITY[RS_FLAG]
    n = 255 - P + 1
    assert RS.codewords(n, P) == 2 and RS.codewords(n - 1, P) == 1
    return RS.frame_size(n, P)


@functools.lru_cache(maxsize=2)
def rs_case(A, S, max_frames):
    """POOL groups of rows drawn from the CPU test's cases (lengths 0, 5, the
    last with one codeword, the first with two; every pattern but "parity"), the
    host decoder's rows and records for them over poison, and the slots."""
    W = rs_width()
    rng = np.random.default_rng(S * 10 + max_frames + RS_FLAG)
    P, c = RS.PARITY[RS_FLAG], C.CRC_BYTES[RS_KIND]
    most = RS.max_len(W, RS_H, c, P)
    assert RS.codewords(RS_H + most + c, P) == 2
    cases = np.stack(TR.case_rows(A, RS_FLAG, RS_H, RS_KIND, W, rng, lengths=(0, 5, most - 1, most),
                                  patterns=("none", "one", "t", "t+1", "ends", "header")))
    rows = cases[rng.integers(0, len(cases), (POOL, max_frames))]
    counts = stored_counts(rng, max_frames)
    want = TR.host_stage(A, rows.reshape(POOL * max_frames, W), counts, max_frames, RS_H, RS_KIND, RS_FLAG)
    return W, rows, counts, want, draw_slots(rng, S)


@pytest.mark.parametrize("S,max_frames,most,waves", [GEOMETRY[1], GEOMETRY[4]])
def test_rs_geometry(A, torch, handle, S, max_frames, most, waves):
    """demod_frames_rs_async at parity 16, h 1, CRC-16, rows of 272 bytes (two
    codewords): S = 5461 x 4 rows (3 waves a group, a last block with a wave
    that leaves) and S = 16385 x 3 (the 16384 / S == 0 fallback). Rows and
    records whole against the host decoder over poison, between guard bands;
    the stored counts stay as they were."""
    W, rows, counts, (w_rows, w_rec), idx = rs_case(A, S, max_frames)
    wpg = waves_per_group(S, max_frames)
    assert (MAX_WAVES // S if MAX_WAVES // S else 1) == most and S * wpg == waves
    assert_last_block_holds_rows(S, wpg, idx, counts, max_frames, LIVE.get(S, WAVES_PER_BLOCK))
    statuses = [w_rec[p, :min(counts[p], max_frames)].copy().view(A.FRAME_RS_DTYPE)["status"].reshape(-1)
                for p in range(POOL)]
    stats = tally(S, max_frames, idx, counts, statuses)
    assert set(stats["status"]) == {RS.OK, RS.FAILED, RS.BAD_LENGTH}
    assert not np.array_equal(w_rows, rows)                       # the host decoder corrected bytes
    print(f"rs S={S} max_frames={max_frames}: {stats}")
    d = handle(4, 2)
    N = 8 * W
    assert d._frame_shape(N, RS_H, RS_KIND, RS_FLAG) == (W, RS.max_len(W, RS_H, 2, 16))
    got = TR.run_stage(A, torch, d, rows[idx].reshape(S * max_frames, W), [counts[p] for p in idx], max_frames, N,
                       RS_H, RS_KIND, RS_FLAG)
    TR.same(got, (w_rows[idx], w_rec[idx]), S)


TXG = dict(S=16385, max_frames=3, K=2, n=1024, L=8, h=1, kind=C.CRC16, gap=2, max_len=2)


def host_encoder(A, x, K):
    """tx_ref's frame_count and frame_symbols by the host encoder
    (demod_tx_frame_symbols, which tests/test_tx_cpu.py and tests/test_rs_cpu.py
    hold to the references): every mode, the parity flags among them."""
    memo = {}

    def symbols(c, data):
        data = bytes(data)
        if data not in memo:
            memo[data] = np.asarray(A.tx_frame_symbols(x, K, data), np.uint8)
        return memo[data]

    return (lambda c, length: len(symbols(c, bytes(length)))), symbols


@pytest.mark.parametrize("fec", [0, RS.FLAG16])
def test_tx_encode_geometry(A, torch, handle, monkeypatch, fec):
    """demod_tx_encode_async at n_streams = 16385 (one wave a stream: the 16384
    / S == 0 fallback), max_frames 3, a ring of three shortest frames and their
    gaps, in a plain mode and with parity 16: places, states and rings whole
    against tests/tx_ref.py's send over the host encoder's symbols, between
    guard bands; records, counts and bytes as they were. Stored counts 0, 3,
    above 3 and 2^32 - 1. The host encoder takes a frame's span from the same
    frame_air_symbols (csrc/frame_shape.h) as the write kernel: the span is
    independent of the device code through the CPU tests named above alone,
    and through this test's passing on the commit before the span was shared."""
    g = TXG
    S, mf, K = g["S"], g["max_frames"], g["K"]
    assert waves_per_group(S, mf) == 1 and last_block(S, 1)[0] == LIVE[S]
    word = (np.arange(g["L"]) * 5 // 3) % K
    c = T.make(T.loop_tones(K), g["n"], [0], word, h=g["h"], kind=g["kind"], fec=fec, max_len=g["max_len"],
               gap=g["gap"], idle=(1, 0, 1), max_frames=mf, stride=2880, ring=1)
    x = A.make_tx_cfg(c.sync, c.h, c.kind, c.fec, c.max_len, c.gap, c.idle, c.amplitude, c.sigma, c.seed, 1, mf,
                      c.stride)
    count_fn, symbols_fn = host_encoder(A, x, K)
    monkeypatch.setattr(T, "frame_count", count_fn)
    monkeypatch.setattr(T, "frame_symbols", symbols_fn)
    c.C = 3 * (T.frame_count(c, 0) + c.gap)
    x.ring_symbols = c.C
    rng = np.random.default_rng(S + fec)
    state = TT.random_state(c, POOL, rng)
    state["tail"][:8] = state["head"][:8]                          # empty rings: three shortest frames fit
    state["offset"][:8] = 0
    records = np.zeros((POOL, mf), T.RECORD_DTYPE)
    records["length"] = rng.choice([0, 0, 1, c.max_len, c.max_len + 1], (POOL, mf))
    records["length"][0] = 0                                       # pool entry 0: all three accepted
    data = rng.integers(0, 256, 64).astype(np.uint8)
    records["body"] = rng.integers(0, data.size + 3, (POOL, mf))
    count = np.array(stored_counts(rng, mf), np.uint64)
    count[3] = 2 ** 32 - 1
    count = count.astype(np.uint32)
    idx = draw_slots(rng, S)
    for poison in TT.POISONS:
        ring = np.full((POOL, c.C), poison, np.uint8)
        place0 = TT.poisoned((POOL, mf), T.PLACE_DTYPE, poison)
        w_state, w_ring, w_place = T.send(c, state, ring, records, count, data, place0)
        assert (w_place["status"][0] == T.OK).all()
        assert {int(v) for p in range(POOL) for v in w_place["status"][p, :min(int(count[p]), mf)]} == \
            {T.OK, T.BAD_LENGTH, T.NO_ROOM}
        o = TT.Outs(torch, poison)
        d_state = o.u8(S * 40, init=state[idx])
        d_ring = o.u8(S * c.C, init=ring[idx])
        d_place = o.u8(S * mf * 16)
        ins = [records[idx].view(np.uint8).reshape(-1), count[idx].view(np.uint8), data]
        d_in = [torch.from_numpy(a.copy()).cuda() for a in ins]
        handle(4, K).tx_encode_async(x, d_state, d_ring, d_in[0], d_in[1].view(torch.int32), d_in[2], data.size, S,
                                     d_place)
        o.guards_intact()
        TT.same(TT.host(d_place, np.uint8), w_place[idx].view(np.uint8), (fec, poison, "place"))
        TT.same(TT.host(d_state, np.uint8), w_state[idx].view(np.uint8), (fec, poison, "state"))
        TT.same(TT.host(d_ring, np.uint8), w_ring[idx], (fec, poison, "ring"))
        for t, a in zip(d_in, ins):
            TT.same(t.cpu().numpy(), a, "an input was written to")


RXG = dict(S=16385, K=2, L=8, max_len=1, max_frames=2, pool=12, loaded=0.04)


@functools.lru_cache(maxsize=1)
def rx_push_case(A, d):
    """One push's packets as a pool of 12: none (entries 1, 5, 9), a cut of a
    one-frame recording (entry 0: all of it) and a two-frame recording behind
    some noise, more windows than the ring holds: its first frame is lost to
    the overflow. What the reference receiver (tests/rx_ref.py, on the
    detector's own outputs) returns for each, and the slots: most streams push
    nothing, about one in 25 a drawn entry."""
    g = RXG
    S, K, L = g["S"], g["K"], g["L"]
    rng = np.random.default_rng(S)
    word = np.array([1, 1, 0, 1, 0, 0, 1, 0], np.uint8)
    Nsym = RX.row_symbols(TX.H, TX.KIND, 0, 1, g["max_len"])
    ring = RX.min_ring(L, Nsym, TX.R)
    short = RX.synth_pcm(TX.tones(K), RX.stream_symbols([4, b"\x5a", 5], K, word, TX.H, TX.KIND, 0, rng)[0], TX.N, 99)
    long = RX.synth_pcm(TX.tones(K), RX.stream_symbols([30, b"\xc3", 3, b"", 12], K, word, TX.H, TX.KIND, 0, rng)[0],
                        TX.N, 98)
    assert (len(short) - TX.N) // TX.HOP + 1 < ring < (len(long) - TX.N) // TX.HOP + 1
    packets, want, states = [], [], []
    for p in range(g["pool"]):
        if p % 4 == 1:
            pk = None
        elif p % 4 == 3:
            pk = np.concatenate([rng.integers(-300, 301, 100 + 256 * (p // 4)).astype(np.int16), long])
        else:
            pk = short[:int(rng.integers(TX.N, len(short) + 1))] if p else short
        ref = RX.Rx(1, K, TX.R, word, 0, Nsym, TX.H, TX.KIND, 0, g["max_frames"], ring)
        piece = None
        if pk is not None:
            Wp = (len(pk) - TX.N) // TX.HOP + 1
            sym, P = d.batch(pk[:(Wp - 1) * TX.HOP + TX.N], mags=True)
            piece = (sym, P)
            assert (Wp > ring) == (p % 4 == 3)
        fr, bodies, summ = ref.push([piece])
        packets.append(pk)
        want.append((fr, bodies, summ))
        states.append({k: int(ref.state[k][0]) for k in ref.state.dtype.names})
    idx = np.where(rng.random(S) < g["loaded"], rng.integers(0, g["pool"], S), 1)
    idx[0], idx[1], idx[2], idx[S - 1] = 0, 1, 3, 0
    return word, Nsym, ring, packets, want, states, idx


def test_rx_push_geometry(A, torch, handle):
    """demod_rx_push at n_streams = 16385 (the copy launch runs one wave a
    stream: the 16384 / S == 0 fallback), the smallest ring the receiver
    accepts, 2 tones, one push: records, bytes and summary whole against the
    reference receiver per stream, and the state of every one of the 16385
    streams, those that pushed nothing included."""
    g = RXG
    S, K = g["S"], g["K"]
    word, Nsym, ring, packets, want, states, idx = rx_push_case(A, handle(4, K))
    assert row_waves(S, ring * K) == 1 and last_block(S, 1)[0] == LIVE[S]
    assert len(want[0][0]) == 1 and states[3]["dropped"] > 0 and len(want[3][0]) >= 1
    assert states[1] == dict(base=0, hold=0, dropped=0, cut_hits=0, fill=0, keep=0)
    rxcfg = A.make_rx_cfg(word, 0, Nsym, TX.H, TX.KIND, 0, g["max_frames"], ring)
    with pytest.raises(A.DemodError):
        A.rx_sizes(handle(4, K).cfg, A.make_rx_cfg(word, 0, Nsym, TX.H, TX.KIND, 0, g["max_frames"], ring - 1), S)
    frames, bodies, nb, checked, valid = [], [], 0, 0, 0
    for s in np.flatnonzero(idx != 1):
        fr, bo, summ = want[idx[s]]
        for f, b in zip(fr, bo):
            frames.append((s, len(b), int(f["window"]), nb, int(f["errors"]), 0))
            nb += len(b)
        bodies += bo
        checked, valid = checked + summ["n_checked"], valid + summ["n_valid"]
    w_frames = np.array(frames, RX.FRAME_DTYPE).reshape(-1)
    host_packets = [None if packets[p] is None else packets[p].copy() for p in range(g["pool"])]
    with A.Receiver(S, rxcfg, n=TX.N, hop=TX.HOP, freqs=TX.tones(K)) as rx:
        fr, bo, summ = rx.push([packets[p] for p in idx])
        assert fr.tobytes() == w_frames.tobytes() and bo == bodies
        assert summ == dict(n_frames=len(frames), n_bytes=nb, n_checked=checked, n_valid=valid)
        for s in range(S):
            assert rx.state(s) == states[idx[s]], s
    for a, b in zip(packets, host_packets):
        assert a is None or np.array_equal(a, b), "a packet was written to"
    print(f"rx push S={S} ring={ring}: {len(frames)} frames of {int((idx != 1).sum())} loaded streams, "
          f"{int((idx % 4 == 3).sum())} of them past the ring")


def row_waves(S, elements):
    """waves a group of a launch that moves `elements` 4-byte words a group"""
    most = MAX_WAVES // S if MAX_WAVES // S else 1
    return min(-(-elements // LANES), most)
