"""The segmented frame scan on the GPU (acquire_frames_segments.hip) against
tests/frames_segments_ref.py: S segments of one batch, each scanned as a batch
of its own, in one call.

Kernel level: test-made sym / P on the device. Everything is compared by
equality: the powers are small integers, so every order of summing them is
exact and the metric's bytes are the reference's too; where the powers are
arbitrary floats (14 decades) the phase fields are compared with
demod_acquire_segments_async's, byte for byte, as include/demod.h promises.
Every call runs with d_hits, d_payload, d_packed, d_results and d_work between
poisoned guards.

End to end: twelve recordings in one batch through the sliding plain bank, the
fold-slide and the FFT; the n / 2 slip as two segments; a captured graph
replayed after its tables were rewritten in place.
"""
import functools

import numpy as np
import pytest

import acquire_ref as AR
import acquire_segments_ref as SR
import frames_ref as F
import frames_segments_ref as FS
import guards as G
from test_gpu_frames import SHAPE_OF_R, float_inputs, make_inputs, plant
from gpu_support import (LEAD, check_frames as check, frames_result_bytes as result_bytes, guarded, handle_fixture,
                         parse_frames as parse, phased, tables, tones_375, torch)  # noqa: F401

pytestmark = pytest.mark.gpu

RS, KS = (1, 4, 64), (1, 2, 16)
RES_BYTES = F.RESULT_DTYPE.itemsize
ARES_BYTES = AR.RESULT_DTYPE.itemsize
PREFIX = F.RESULT_DTYPE.fields["n_hits"][1]     # metric[64], phases, phase, per_phase: as demod_acquire_result_t
HIT = 16


# handle(R, K): one Demodulator per (R, K), closed with the module.
handle = handle_fixture(lambda A, Rn, K: phased(A, SHAPE_OF_R, Rn, tones_375(K)))


class Runner:
    """Device buffers of one (handle, batch). run() puts every output and the
    workspace between poisoned guards, checks them and returns one dict per
    segment: the raw result, its parse and the segment's rows whole, rows past
    n_written included."""

    def __init__(self, A, torch, d, sym, P):
        self.A, self.torch, self.d = A, torch, d
        self.Wb, self.K = len(sym), P.shape[1]
        self.bits = F.bits_per_symbol(self.K)
        self.d_sym = torch.from_numpy(np.ascontiguousarray(sym)).cuda()
        self.d_P = torch.from_numpy(np.ascontiguousarray(P)).cuda()
        self.g_work = None

    def run(self, first, count, word, me, N, cap, payload=True, packed=True, stream=0, sym=None,
            poison=0xFF, work_windows=None, work_bytes=None, work_poison=0xFF, n_windows=None):
        A, torch = self.A, self.torch
        S = len(first)
        if sym is not None:
            self.d_sym.copy_(torch.from_numpy(sym))
        Wb = self.Wb if n_windows is None else n_windows
        B = (N * self.bits + 7) // 8
        d_first, d_count = tables(torch, first, count)
        g_hits, chk_hits = guarded(torch, S * cap * HIT, LEAD, poison)
        g_pay, chk_pay = guarded(torch, S * cap * N if payload else 0, LEAD + 1, poison)
        g_pak, chk_pak = guarded(torch, S * cap * B if packed else 0, LEAD + 3, poison)
        g_res, chk_res = guarded(torch, S * RES_BYTES, LEAD, poison)
        wb = work_bytes if work_bytes is not None else A.frames_segments_workspace_size(
            self.d.cfg, S, Wb if work_windows is None else work_windows)
        if work_poison is None and self.g_work is not None and self.g_work[0].numel() == wb:
            g_work, chk_work = self.g_work                 # as the call before left it
        else:
            g_work, chk_work = guarded(torch, wb, LEAD, 0xFF)
            g_work.fill_(0xFF if work_poison is None else work_poison)
        self.g_work = (g_work, chk_work)
        self.d.frames_segments_async(self.d_sym, self.d_P, Wb, d_first, d_count, S, word, me, N, g_hits,
                                     g_pay, g_pak, cap, g_res, g_work, stream=stream)
        for chk in (chk_hits, chk_pay, chk_pak, chk_res):
            chk(written=False)
        # the work guards: poison 0xFF whatever the body was filled with
        torch.cuda.synchronize()
        chk_work(written=False)
        raw = g_res.cpu().numpy().tobytes()

        def rows(t, width):
            return (t.cpu().numpy().reshape(S, cap, width) if t is not None
                    else np.zeros((S, cap, width), np.uint8))
        hits, pay, pak = rows(g_hits, HIT), rows(g_pay, N), rows(g_pak, B)
        out = []
        for s in range(S):
            r = raw[s * RES_BYTES:(s + 1) * RES_BYTES]
            out.append(dict(raw=r, res=parse(A, r), hits=np.ascontiguousarray(hits[s]).reshape(-1).view(F.HIT_DTYPE),
                            payload=pay[s] if g_pay is not None else None,
                            packed=pak[s] if g_pak is not None else None))
        return out


def check_all(A, outs, refs, cap, poison=0xFF):
    assert len(outs) == len(refs)
    for s, (o, r) in enumerate(zip(outs, refs)):
        try:
            check(A, o, r, cap, poison)
        except AssertionError as e:
            raise AssertionError(f"segment {s}: {e}") from e


def layout(counts, gap, lead=0):
    first, at = [], lead
    for c in counts:
        first.append(at)
        at += c + gap
    return first, max(at - gap, 1)


def fill(Wb, K, Rn, first, count, seed, gap_poison=False, targets=None):
    """A batch whose segments hold test_gpu_frames.make_inputs contents of
    their own (small integer powers, phase targets[s], default (s + 1) % R,
    eight times as large, relative to the segment) and whose other windows are
    random, or (gap_poison) sym 0xFF with P alternately NaN and 3e38."""
    sym, P = make_inputs(Wb, K, Rn, seed, 0)
    if gap_poison:
        sym[:] = 0xFF
        P[0::2] = np.float32(np.nan)
        P[1::2] = np.float32(3e38)
    for s, (f, c) in enumerate(zip(first, count)):
        if c:
            t = (s + 1) % Rn if targets is None else targets[s]
            sym[f:f + c], P[f:f + c] = make_inputs(c, K, Rn, seed + 100 + s, t)
    return sym, P


def slices_agree(A, torch, d, run, first, count, word, me, N, cap, outs):
    """demod_frames_async on each slice of at least R windows: the same result
    bytes (the powers are integers: every order of summing is exact) and rows."""
    Rn = d.n // d.hop
    B = (N * run.bits + 7) // 8
    d_res = torch.empty(RES_BYTES, dtype=torch.uint8, device="cuda")
    done = 0
    for s, (f, c) in enumerate(zip(first, count)):
        f, c = SR.clamp(f, c, run.Wb)
        if c < Rn:
            continue
        d_work = torch.empty(A.frames_workspace_size(d.cfg, c), dtype=torch.uint8, device="cuda")
        bufs = [torch.full((max(cap * w, 1),), 0xFF, dtype=torch.uint8, device="cuda") for w in (HIT, N, B)]
        d.frames_async(run.d_sym[f:f + c], run.d_P[f:f + c].reshape(-1), c, word, me, N, bufs[0],
                       bufs[1] if N else None, bufs[2] if N else None, cap, d_res, d_work)
        torch.cuda.synchronize()
        o = outs[s]
        assert d_res.cpu().numpy().tobytes() == o["raw"], s
        nw = o["res"]["n_written"]
        assert bufs[0].cpu().numpy()[:nw * HIT].tobytes() == o["hits"][:nw].tobytes()
        if N:
            assert np.array_equal(bufs[1].cpu().numpy()[:nw * N].reshape(nw, N), o["payload"][:nw])
            assert np.array_equal(bufs[2].cpu().numpy()[:nw * B].reshape(nw, B), o["packed"][:nw])
        done += 1
    return done


def phase_fields_agree(A, torch, d, Wb, K, Rn, first, count, word, me, N):
    """Arbitrary float powers over 14 decades: metric, phases, phase and
    per_phase of every segment are demod_acquire_segments_async's bytes."""
    fsym, fP = float_inputs(Wb, K, Rn, 3 * Rn + K, 1 % Rn)
    frun = Runner(A, torch, d, fsym, fP)
    fgot = frun.run(first, count, word, me, N, 4)
    S = len(first)
    d_first, d_count = tables(torch, first, count)
    d_ares = torch.empty(S * ARES_BYTES, dtype=torch.uint8, device="cuda")
    d_awork = torch.empty(A.acquire_segments_workspace_size(d.cfg, S, Wb), dtype=torch.uint8, device="cuda")
    d.acquire_segments_async(frun.d_sym, frun.d_P, Wb, d_first, d_count, S, word, me, None, d_ares, d_awork)
    torch.cuda.synchronize()
    araw = d_ares.cpu().numpy().tobytes()
    for s in range(S):
        assert fgot[s]["raw"][:PREFIX] == araw[s * ARES_BYTES:s * ARES_BYTES + PREFIX], s


# ---- 1. equivalence ----------------------------------------------------------

@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("Rn", RS)
def test_equivalence(A, torch, handle, Rn, K):
    """Nine segments around R and around the tile, shuffled; touching, with gaps
    of R - 1 windows, and with `first` reversed: every byte equals the
    reference's and demod_frames_async's on the slice; on 14-decade float
    powers the four phase fields are demod_acquire_segments_async's bytes."""
    T = A.ACQUIRE_TILE
    d = handle(Rn, K)
    counts = [0, Rn - 1, Rn, Rn + 1, T - 1, T, T + 1, 2 * T + 5, 3]
    counts = [counts[i] for i in np.random.default_rng(Rn * 31 + K).permutation(len(counts))]
    word = ((np.arange(5) * 3 + 1) % K).astype(np.uint8)
    L, N, me = len(word), 7, 1
    hits_seen = tails_seen = 0
    for variant, gap in (("touching", 0), ("gaps", Rn - 1), ("reversed", Rn - 1)):
        first, Wb = layout(counts, gap)
        count = list(counts)
        if variant == "reversed":      # the same slices listed from the last to the first
            first, count = first[::-1], count[::-1]
        sym, P = fill(Wb, K, Rn, first, count, 7 * Rn + K)
        # on each segment's boosted phase: the word with one mismatch in mid-segment, and a
        # clean one whose payload runs past the segment's end (the tail)
        for s, (f, c) in enumerate(zip(first, count)):
            ph = (s + 1) % Rn
            if c >= 2 * (L + N + 2) * Rn:
                plant(sym, Rn, K, f + ph + (c // Rn // 2 - L - N) * Rn, word, me, salt=s)
                last = (c - 1 - ph) // Rn * Rn + ph              # the phase's last window
                plant(sym, Rn, K, f + last - (L + 2) * Rn, word, 0)
        run = Runner(A, torch, d, sym, P)
        want = FS.frames_segments(sym, P, Rn, first, count, word, me, N)
        cap = max(r[3]["n_hits"] for r in want) + 2
        got = run.run(first, count, word, me, N, cap)
        check_all(A, got, want, cap)
        assert slices_agree(A, torch, d, run, first, count, word, me, N, cap, got) == sum(
            c >= Rn for c in counts)
        hits_seen += sum(r[3]["n_hits"] for r in want)
        tails_seen += sum(r[3]["tail_window"] >= 0 for r in want)
        phase_fields_agree(A, torch, d, Wb, K, Rn, first, count, word, me, N)
    assert hits_seen >= 3 and tails_seen >= 3


# ---- 2. boundaries -----------------------------------------------------------

@pytest.mark.parametrize("Rn,K,me,gap", [(1, 2, 0, 0), (4, 16, 2, 0), (4, 2, 1, 3), (64, 2, 3, 0),
                                         (64, 16, 0, 63)])
def test_boundaries(A, torch, handle, Rn, K, me, gap):
    """A 24-symbol word with exactly max_errors mismatches, on each segment's
    phase: at the last complete start it is a hit; one start later it is the
    tail, not a hit; split across a segment boundary, whichever way, it is
    absent from both sides; across a tile edge inside a segment it is a hit; on
    another phase it is absent. The windows between segments (gap > 0) hold
    NaN / 3e38 powers and 0xFF symbols."""
    T, L, N = A.ACQUIRE_TILE, 24, 3
    span = (L + N - 1) * Rn
    big = 2 * T if Rn < 64 else 4 * T
    counts = [big + 5 * Rn + 1, big, (L + N + 6) * Rn + 1, (L + N + 2) * Rn]
    S = len(counts)
    first, Wb = layout(counts, gap, lead=3 if gap else 0)
    rng = np.random.default_rng(Rn * 5 + K)
    word = rng.integers(0, K, L).astype(np.uint8)
    if K > 1:
        word[::2] = (word[1::2] + 1) % K          # no run: a shifted copy is far from the word
    sym, P = fill(Wb, K, Rn, first, counts, 40 + Rn + K, gap_poison=gap > 0)
    if K > 1:
        sym[sym < K] = (word[0] + 1) % K          # a background with nothing near the word
    else:
        sym[:] = 0xFF
    d = handle(Rn, K)
    run = Runner(A, torch, d, sym, P)
    base = FS.frames_segments(sym, P, Rn, first, counts, word, me, N)
    phase = [r[3]["phase"] for r in base]
    assert phase == [(s + 1) % Rn for s in range(S)]
    assert all(r[3]["n_hits"] == 0 and r[3]["tail_window"] == -1 for r in base)
    cap = 4
    check_all(A, run.run(first, counts, word, me, N, cap), base, cap)

    def go(s2):
        want = FS.frames_segments(s2, P, Rn, first, counts, word, me, N)
        check_all(A, run.run(first, counts, word, me, N, cap, sym=s2), want, cap)
        return [(r[0]["window"].tolist(), r[3]["tail_window"]) for r in want]

    def put(s2, s, w, n_bad, salt=0):
        plant(s2, Rn, K, first[s] + w, word, n_bad, salt=salt)

    nothing = [([], -1)] * S
    for s in range(S):
        c, ph = counts[s], phase[s]
        last = (c - 1 - span - ph) // Rn * Rn + ph              # the last complete start
        assert last + span < c <= last + Rn + span
        # the last complete start: a hit; with one more mismatch: nothing
        s2 = sym.copy()
        put(s2, s, last, me, salt=s)
        assert go(s2) == [([last], -1) if j == s else ([], -1) for j in range(S)]
        if me + 1 < L and K > 1:
            s2 = sym.copy()
            put(s2, s, last, me + 1, salt=s)
            assert go(s2) == nothing
        # one start later: the word fits, the payload does not: the tail
        s2 = sym.copy()
        put(s2, s, last + Rn, me, salt=s + 1)
        assert go(s2) == [([], last + Rn) if j == s else ([], -1) for j in range(S)]
        # on the next phase: absent
        if Rn > 1:
            s2 = sym.copy()
            put(s2, s, last - Rn + 1 if ph + 1 < Rn else last - Rn - ph, 0)
            assert go(s2) == nothing
        # across a tile edge inside the segment, at three splits
        edge = T if (L - 1) * Rn <= T else 2 * T                 # (R = 64: the word is longer than a tile)
        if c > edge + span:
            for i in (1, L // 2, L - 1):
                w = edge - i * Rn + ph
                s2 = sym.copy()
                put(s2, s, w, me, salt=i)
                assert 0 <= w < edge <= w + (L - 1) * Rn
                assert go(s2) == [([w], -1) if j == s else ([], -1) for j in range(S)]
    # the word across each boundary: its first i symbols end segment s, the rest start s + 1
    for s in range(S - 1):
        tail = first[s] + np.arange(phase[s], counts[s], Rn)
        head = first[s + 1] + np.arange(phase[s + 1], counts[s + 1], Rn)
        for i in range(1, L):
            s2 = sym.copy()
            s2[tail[len(tail) - i:]] = word[:i]
            s2[head[:L - i]] = word[i:]
            assert go(s2) == nothing, (s, i)


@pytest.mark.parametrize("Rn,K", [(1, 2), (4, 16), (64, 2)])
def test_payload_reach(A, torch, handle, Rn, K):
    """A payload that reaches exactly the segment's last window is complete; one
    window further is the tail. Segments with gaps of NaN / 3e38 powers and
    0xFF symbols, the phase chosen so that its last window is the segment's."""
    T, L, N, me = A.ACQUIRE_TILE, 24, 64, 2
    span = (L + N - 1) * Rn
    counts = [span + T + 3, span + 1, span + 2 * T, span + Rn + 1]     # the hit at T + 2, 0, 2 T - 1, R
    S = len(counts)
    first, Wb = layout(counts, 5, lead=2)
    targets = [(c - 1) % Rn for c in counts]
    sym, P = fill(Wb, K, Rn, first, counts, 70 + Rn, gap_poison=True, targets=targets)
    rng = np.random.default_rng(Rn + K)
    word = rng.integers(0, K, L).astype(np.uint8)
    word[::2] = (word[1::2] + 1) % K
    sym[sym < K] = (word[0] + 1) % K
    run = Runner(A, torch, handle(Rn, K), sym, P)
    for shift, hit in ((0, True), (1, False)):
        s2 = sym.copy()
        at = []
        for s, c in enumerate(counts):
            w = c - 1 - span
            assert w % Rn == targets[s]
            # one start later on the phase: the last payload symbol would be R windows past the end
            w2 = w + shift * Rn
            at.append(w2)
            plant(s2, Rn, K, first[s] + w2, word, me, salt=s)
            s2[first[s] + w2 + L * Rn:first[s] + c:Rn] = (np.arange(len(range(w2 + L * Rn, c, Rn))) % K)
        want = FS.frames_segments(s2, P, Rn, first, counts, word, me, N)
        got = run.run(first, counts, word, me, N, 2, sym=s2)
        check_all(A, got, want, 2)
        for s in range(S):
            assert want[s][3]["phase"] == targets[s]
            if hit:
                assert got[s]["hits"]["window"][:1].tolist() == [at[s]] and got[s]["res"]["tail_window"] == -1
                assert got[s]["payload"][0, -1] == s2[first[s] + counts[s] - 1]
            else:
                assert got[s]["res"]["n_hits"] == 0 and got[s]["res"]["tail_window"] == at[s]
                assert got[s]["res"]["tail_errors"] == me


# ---- 3. max_frames -----------------------------------------------------------

@pytest.mark.parametrize("Rn", RS)
def test_max_frames(A, torch, handle, Rn):
    """K = 1, L = 1, all symbols 0: every start on the phase is a hit. Three
    segments with different hit counts; max_frames 0, 1, one segment's exact
    count and one more: the counts stay, the rows are cut, rows past n_written
    keep their poison and no segment writes a neighbour's rows."""
    T, K, N = A.ACQUIRE_TILE, 1, 7
    counts = [T + 5 * Rn + 1, 3 * T + 7, 12 * Rn]
    first, Wb = layout(counts, 2)
    sym = np.zeros(Wb, np.uint8)
    P = np.ones((Wb, 1), np.float32)
    for s, (f, c) in enumerate(zip(first, counts)):
        P[f + (s + 1) % Rn:f + c:Rn] = 8.0
    word = np.zeros(1, np.uint8)
    want = FS.frames_segments(sym, P, Rn, first, counts, word, 0, N)
    n_hits = [r[3]["n_hits"] for r in want]
    for s, c in enumerate(counts):
        starts = np.arange((s + 1) % Rn, c, Rn)
        assert n_hits[s] == int(np.count_nonzero(starts + N * Rn < c))
        assert want[s][3]["tail_window"] == starts[n_hits[s]]
    exact = n_hits[2]
    assert 1 < exact < min(n_hits[:2])
    run = Runner(A, torch, handle(Rn, K), sym, P)
    for cap in (0, 1, exact, exact + 1, max(n_hits) + 3):
        got = run.run(first, counts, word, 0, N, cap, poison=0x5A)
        check_all(A, got, want, cap, 0x5A)
        assert [o["res"]["n_hits"] for o in got] == n_hits
        assert [o["res"]["n_written"] for o in got] == [min(cap, n) for n in n_hits]
    # payload alone, packed alone, neither
    cap = exact + 1
    for pay, pak in ((True, False), (False, True), (False, False)):
        got = run.run(first, counts, word, 0, N, cap, payload=pay, packed=pak)
        check_all(A, got, want, cap)
        assert (got[0]["payload"] is None) == (not pay) and (got[0]["packed"] is None) == (not pak)
    got = run.run(first, counts, word, 0, 0, cap)                # N = 0: the word is the frame
    check_all(A, got, FS.frames_segments(sym, P, Rn, first, counts, word, 0, 0), cap)


# ---- 4. position independence -------------------------------------------------

@pytest.mark.parametrize("Rn,K", [(4, 2), (64, 2), (1, 16)])
def test_position_independence(A, torch, handle, Rn, K):
    """One segment's contents (14-decade float powers) at three places, in slots
    0, 1 and S - 1, beside different neighbours, S in {1, 3, 1025}, and on a
    second stream: the same result bytes and the same rows every time."""
    T, N, me = A.ACQUIRE_TILE, 16, 1
    c0 = 2 * T + 37 * Rn + 3
    seg_sym, seg_P = float_inputs(c0, K, Rn, 99 + Rn, Rn // 2)
    word = np.array([1, 0, 1], np.uint8) % K
    ref = F.frames(seg_sym, seg_P, Rn, word, me, N)
    cap = ref[3]["n_hits"] + 2
    assert ref[3]["n_hits"] > 10
    d = handle(Rn, K)
    seen = []
    side = torch.cuda.Stream()
    for S, slots in ((1, (0,)), (3, (0, 1, 2)), (1025, (0, 1, 1024))):
        for slot in slots:
            rng = np.random.default_rng(1000 * S + slot)
            counts = [int(v) for v in rng.integers(0, 40, S)]
            counts[slot] = c0
            first, Wb = layout(counts, int(rng.integers(0, 5)), lead=int(rng.integers(0, 3000)))
            sym, P = float_inputs(Wb, K, Rn, S + slot, 0)
            sym[first[slot]:first[slot] + c0] = seg_sym
            P[first[slot]:first[slot] + c0] = seg_P
            run = Runner(A, torch, d, sym, P)
            got = run.run(first, counts, word, me, N, cap)
            o = got[slot]
            if o["res"]["phase"] == ref[3]["phase"]:       # (the GPU's own order of float sums)
                assert o["res"]["n_hits"] == ref[3]["n_hits"]
                assert o["hits"][:ref[3]["n_hits"]].tobytes() == ref[0].tobytes()
                assert np.array_equal(o["payload"][:ref[3]["n_hits"]], ref[1])
            seen.append((o["raw"], o["hits"].tobytes(), o["payload"].tobytes(), o["packed"].tobytes()))
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                got2 = run.run(first, counts, word, me, N, cap, stream=side.cuda_stream)
            for a, b in zip(got, got2):
                assert a["raw"] == b["raw"] and a["hits"].tobytes() == b["hits"].tobytes()
                assert a["payload"].tobytes() == b["payload"].tobytes()
    assert len(seen) == 7 and all(v == seen[0] for v in seen)


# ---- 5. long segments: the finaliser's workgroup path -------------------------

@pytest.mark.parametrize("Rn,K", [(4, 2), (64, 16), (1, 2)])
def test_long_segments(A, torch, handle, Rn, K):
    """Segments of 66 tiles take the finaliser's workgroup path (sums, tail and
    the prefix in chunks): hits in tiles 0, 63, 64 and 65 of segment X, and a
    second long segment Y overlapping it in the same workgroup's four slots, in
    two layouts. The reference's bytes; X's bytes the same in both places."""
    T, L, N, me = A.ACQUIRE_TILE, 8, 5, 1
    c0 = 66 * T + 5
    ph = Rn // 2
    seg_sym, seg_P = make_inputs(c0, K, Rn, 50 + Rn, ph)
    a = 1
    word = np.array([a, a, a, 0, a, 0, a, a], np.uint8)
    seg_sym[ph::Rn] = 0                      # nothing near the word on the phase
    planted = []
    for tile in (0, 63, 64, 65):
        w = ph + tile * T // Rn * Rn
        plant(seg_sym, Rn, K, w, word, me, salt=tile)
        planted.append(w)
    tail = (c0 - 1 - ph) // Rn * Rn + ph - (L - 1) * Rn      # the last start whose word fits
    plant(seg_sym, Rn, K, tail, word, 0)
    ref = F.frames(seg_sym, seg_P, Rn, word, me, N)
    assert ref[3]["phase"] == ph and ref[0]["window"].tolist() == planted
    assert [w // T for w in planted] == [0, 63, 64, 65] and ref[3]["tail_window"] == tail
    cap = 6
    d = handle(Rn, K)
    rng = np.random.default_rng(7 + Rn)
    seen = []
    for S, sx, sy, lead in ((4, 1, 3, 1500), (6, 0, 2, 707)):
        Wb = lead + c0 + 900
        sym, P = make_inputs(Wb, K, Rn, 60 + S, 0)
        sym[lead:lead + c0], P[lead:lead + c0] = seg_sym, seg_P
        first = [int(v) for v in rng.integers(0, Wb - 50, S)]
        count = [int(v) for v in rng.integers(0, 50, S)]
        first[sx], count[sx] = lead, c0
        first[sy], count[sy] = lead - 700, 66 * T
        want = FS.frames_segments(sym, P, Rn, first, count, word, me, N)
        assert want[sy][3]["per_phase"] == 66 * T // Rn and want[sy][3]["n_hits"] >= 3
        run = Runner(A, torch, d, sym, P)
        got = run.run(first, count, word, me, N, cap, work_windows=3 * Wb)   # overlapping: a wider budget
        check_all(A, got, want, cap)
        check(A, got[sx], ref, cap)
        seen.append((got[sx]["raw"], got[sx]["hits"].tobytes(), got[sx]["payload"].tobytes()))
    assert seen[0] == seen[1]


# ---- 6. the most segments ------------------------------------------------------

def test_max_segments(A, torch, handle):
    """DEMOD_MAX_SEGMENTS segments of 0, 1 or 2 windows at R = 1, L = 1, K = 1,
    all symbols 0: every window is a hit (the all-hit case), more tiles than the
    scan's grid has waves. N = 1: a segment of two has one complete hit, at
    window 0 with the symbol at window 1, and the tail at 1; a segment of one
    has the tail at 0. Checked in closed form for every segment, and the closed
    form against the reference on a sample."""
    Rn, K, cap, N = 1, 1, 2, 1
    S = A.DEMOD_MAX_SEGMENTS
    assert F.RESULT_DTYPE.itemsize == RES_BYTES
    rng = np.random.default_rng(65536)
    count = rng.integers(0, 3, S)
    first = np.cumsum(count + rng.integers(0, 2, S)) - count
    Wb = int(first[-1] + count[-1]) + 3
    assert int((count > 0).sum()) > 4 * 2048                      # tiles > the grid's waves
    sym = np.zeros(Wb, np.uint8)
    P = rng.integers(1, 1024, (Wb, 1)).astype(np.float32)
    word = np.zeros(1, np.uint8)
    run = Runner(A, torch, handle(Rn, K), sym, P)
    d_first, d_count = tables(torch, first, count)
    g_hits, chk_hits = guarded(torch, S * cap * HIT, LEAD, 0xFF)
    g_pay, chk_pay = guarded(torch, S * cap * N, LEAD + 1, 0xFF)
    g_pak, chk_pak = guarded(torch, S * cap * 1, LEAD + 3, 0xFF)
    g_res, chk_res = guarded(torch, S * RES_BYTES, LEAD, 0xFF)
    g_work, chk_work = guarded(torch, A.frames_segments_workspace_size(run.d.cfg, S, Wb), LEAD, 0xFF)
    run.d.frames_segments_async(run.d_sym, run.d_P, Wb, d_first, d_count, S, word, 0, N, g_hits, g_pay,
                                g_pak, cap, g_res, g_work)
    for chk in (chk_hits, chk_pay, chk_pak, chk_res, chk_work):
        chk(written=False)
    res = np.frombuffer(g_res.cpu().numpy().tobytes(), F.RESULT_DTYPE)
    hits = g_hits.cpu().numpy().view(F.HIT_DTYPE).reshape(S, cap)
    pay, pak = g_pay.cpu().numpy().reshape(S, cap), g_pak.cpu().numpy().reshape(S, cap)
    pw = P[:, 0].astype(np.float64)
    w1 = np.minimum(first + 1, Wb - 1)
    M = np.where(count > 0, pw[first], 0.0) + np.where(count > 1, pw[w1], 0.0)
    two = count == 2
    assert np.array_equal(res["metric"][:, 0], M) and not res["metric"][:, 1:].any()
    assert (res["phases"] == 1).all() and not res["phase"].any() and not res["reserved"].any()
    assert np.array_equal(res["per_phase"], count)
    assert np.array_equal(res["n_hits"], two.astype(np.uint64)) and np.array_equal(res["n_written"], res["n_hits"])
    assert np.array_equal(res["tail_window"], np.where(count > 0, count - 1, -1))
    assert not res["tail_errors"].any()
    raw_hits = hits.view(np.uint8).reshape(S, cap * HIT)
    assert not raw_hits[two, :HIT].any() and (raw_hits[two, HIT:] == 0xFF).all()     # {0, 0, 0}, then poison
    assert (raw_hits[~two] == 0xFF).all()
    assert not pay[two, 0].any() and not pak[two, 0].any()
    assert (pay[two, 1] == 0xFF).all() and (pay[~two] == 0xFF).all() and (pak[~two] == 0xFF).all()
    assert two.sum() > 1000
    pick = np.r_[0:S:211, S - 50:S]
    want = FS.frames_segments(sym, P, Rn, first[pick], count[pick], word, 0, N)
    for s, r in zip(pick, want):
        for f in ("phases", "phase", "per_phase", "n_hits", "n_written", "tail_window", "tail_errors"):
            assert res[f][s] == r[3][f], (s, f)
        assert res["metric"][s, 0] == r[3]["metric"][0]


# ---- 7. the tile budget and unchecked tables -----------------------------------

@pytest.mark.parametrize("Rn,K", [(1, 16), (4, 1), (4, 2), (64, 2)])
def test_budget_and_unchecked_tables(A, torch, handle, Rn, K):
    """Tables no host has checked (first > Wb, first + count > Wb, count = 2^32
    - 1, first = 2^40) and overlapping segments past the workspace's tile
    budget: the segments past the budget come out short, the earlier ones
    exact. A work_bytes cut to fewer tiles cuts earlier. d_work poisoned with
    0xFF, with 0x5A and as the call before left it: the same bytes."""
    T = A.ACQUIRE_TILE
    Wb = 3 * T + 100
    first = [0, Wb + 5, Wb - Rn - 1, 0, 0, 5, T, 0, 1 << 40, Wb, 0]
    count = [0xFFFFFFFF, 10, 100, Wb, Wb, Rn, 2 * T + 1, min(2, Rn), 7, 0xFFFFFFFF, Wb]
    S = len(first)
    budget = SR.budget_for(S, Wb)
    assert budget == 4 + S
    d = handle(Rn, K)
    sym, P = make_inputs(Wb, K, Rn, 17 + Rn, Rn - 1)
    word = sym[Rn - 1 + 8 * Rn:Rn - 1 + 11 * Rn:Rn].copy() % K
    L, N, me = len(word), 6, 1
    want = FS.frames_segments(sym, P, Rn, first, count, word, me, N, budget=budget)
    # by the definitions alone: 4 + 1 + 4 + 4 + 1 = 14 tiles fit the 15, the 3 of segment 6 do
    # not, and nothing after it does
    assert [r[3]["per_phase"] > 0 for r in want] == [True, False] + [True] * 4 + [False] * 5
    assert want[0][3]["n_hits"] > 0
    cap = want[0][3]["n_hits"] + 1
    run = Runner(A, torch, d, sym, P)
    raws = []
    for work_poison in (0xFF, 0x5A, None):
        got = run.run(first, count, word, me, N, cap, work_poison=work_poison)
        check_all(A, got, want, cap)
        raws.append([o["raw"] for o in got])
    assert raws[0] == raws[1] == raws[2]
    # a workspace sized for overlapping callers holds them all; segment 0 does not notice
    full = FS.frames_segments(sym, P, Rn, first, count, word, me, N)
    wide = run.run(first, count, word, me, N, cap, work_windows=4 * Wb)
    check_all(A, wide, full, cap)
    assert full[10][3]["per_phase"] == Wb // Rn and wide[0]["raw"] == raws[0][0]
    # the budget is what work_bytes hold: segment 6 needs tiles 15 .. 17. Eight bytes short of
    # 17 tiles it is still dropped; with 17 it is scanned and the next one-tile segment is not
    head = FS.header_bytes(S)
    for wbytes, fit in ((head + FS.tiles_bytes(17, Rn) - 8, 16), (head + FS.tiles_bytes(17, Rn), 17)):
        assert FS.budget_of(wbytes, Rn, S) == fit
        ref = FS.frames_segments(sym, P, Rn, first, count, word, me, N, budget=fit)
        assert (ref[6][3]["per_phase"] > 0) == (fit == 17) and ref[10][3]["per_phase"] == 0
        got = run.run(first, count, word, me, N, cap, work_bytes=wbytes)
        check_all(A, got, ref, cap)
        assert got[0]["raw"] == raws[0][0]


# ---- 8. refusals -------------------------------------------------------------

def test_refusals(A, torch):
    """Every DEMOD_BAD_ARG case returns without a launch: results, rows and
    workspace stay poison."""
    lib = A.load_library()
    K, W, S, cap, N = 8, 4096, 3, 16, 16
    d = A.Demodulator(n=1024, hop=256, freqs=tuple(1500.0 + 375.0 * i for i in range(K)))
    others = [A.Demodulator(n=1024, hop=384, freqs=(1500.0, 3000.0)),
              A.Demodulator(n=1024, hop=8, freqs=(1500.0, 3000.0))]
    try:
        sym, P = make_inputs(W, K, 4, 1, 0)
        d_sym, d_P = torch.from_numpy(sym).cuda(), torch.from_numpy(P).cuda().reshape(-1)
        d_first, d_count = tables(torch, [0, 1000, 3000], [1000, 2000, 1096])
        wb = A.frames_segments_workspace_size(d.cfg, S, W)
        g_hits, chk_hits = guarded(torch, S * cap * HIT, LEAD, 0xFF)
        g_pay, chk_pay = guarded(torch, S * cap * N, LEAD, 0xFF)
        g_pak, chk_pak = guarded(torch, S * cap * N, LEAD, 0xFF)
        g_res, chk_res = guarded(torch, S * RES_BYTES, LEAD, 0xFF)
        g_work, chk_work = guarded(torch, wb, LEAD, 0xFF)
        good = np.arange(8, dtype=np.uint8)
        bad_sym = np.array([0, K], np.uint8)
        long_word = np.zeros(65, np.uint8)
        ps, pm, pf, pc, ph, pp, pk, pr, pw = (t.data_ptr() for t in (d_sym, d_P, d_first, d_count, g_hits,
                                                                     g_pay, g_pak, g_res, g_work))
        ok = dict(h=d._h, sym=ps, mag=pm, W=W, first=pf, count=pc, S=S, sync=good.ctypes.data, L=8, me=0,
                  N=N, hits=ph, pay=pp, pak=pk, cap=cap, res=pr, work=pw, wb=wb)

        def call(**kw):
            a = dict(ok)
            a.update(kw)
            return lib.demod_frames_segments_async(a["h"], a["sym"], a["mag"], a["W"], a["first"],
                                                   a["count"], a["S"], a["sync"], a["L"], a["me"], a["N"],
                                                   a["hits"], a["pay"], a["pak"], a["cap"], a["res"],
                                                   a["work"], a["wb"], None)

        cases = [
            ("NULL handle", dict(h=None)),
            ("W >= 2^31", dict(W=1 << 31)),
            ("sync_len > 64", dict(sync=long_word.ctypes.data, L=65)),
            ("sync symbol >= K", dict(sync=bad_sym.ctypes.data, L=2)),
            ("max_errors >= sync_len", dict(me=8)),
            ("NULL sync", dict(sync=None)),
            ("sync_len == 0", dict(L=0)),
            ("sync_len == 0, NULL sync", dict(sync=None, L=0)),
            ("(L + N) R >= 2^31", dict(N=2 ** 29 - 8)),
            ("NULL d_symbols", dict(sym=None)),
            ("NULL d_mags", dict(mag=None)),
            ("NULL d_results", dict(res=None)),
            ("NULL d_work", dict(work=None)),
            ("NULL d_hits with max_frames", dict(hits=None)),
            ("NULL d_first", dict(first=None)),
            ("NULL d_count", dict(count=None)),
            ("max_frames >= 2^31", dict(cap=2 ** 31)),
            ("n_segments * max_frames >= 2^31", dict(cap=(2 ** 31 + S - 1) // S)),
            ("n_segments == 0", dict(S=0)),
            ("n_segments > DEMOD_MAX_SEGMENTS", dict(S=A.DEMOD_MAX_SEGMENTS + 1, wb=1 << 40, cap=1)),
            ("work_bytes one short", dict(wb=wb - 1)),
            ("work_bytes 0", dict(wb=0)),
            ("misaligned d_hits", dict(hits=ph + 4)),
            ("misaligned d_results", dict(res=pr + 4)),
            ("misaligned d_work", dict(work=pw + 4)),
            ("misaligned d_first", dict(first=pf + 4)),
            ("misaligned d_count", dict(count=pc + 2)),
            ("n % hop != 0", dict(h=others[0]._h, L=1)),
            ("R > 64", dict(h=others[1]._h, L=1)),
        ]
        for what, kw in cases:
            assert call(**kw) == A.DEMOD_BAD_ARG, what
        # the synchronous call checks its host tables before the detector runs
        x = np.zeros(16 * 1024, np.int16)
        for f, c in [([0, 70], [20, 2]), ([0, 30], [20, 32]), ([62], [4]), ([0], [3])]:
            with pytest.raises(A.DemodError) as e:
                d.frames_segments(x, f, c, good[:2])                # 61 windows, R = 4
            assert e.value.code == A.DEMOD_BAD_ARG, (f, c)
        with pytest.raises(A.DemodError) as e:
            d.frames_segments(x, [0], [20], None)                   # no word
        assert e.value.code == A.DEMOD_BAD_ARG
        for dd in others:
            with pytest.raises(A.DemodError) as e:
                dd.frames_segments(x, [0], [8], good[:2])
            assert e.value.code == A.DEMOD_BAD_ARG
        # the Python mirror's own checks (before any pointer reaches the library)
        base = dict(d_sym=d_sym, d_mag=d_P, d_first=d_first, d_count=d_count, d_hits=g_hits, d_payload=g_pay,
                    d_packed=g_pak, d_results=g_res, d_work=g_work)
        for kw in (dict(d_sym=d_sym[:W - 1]), dict(d_mag=d_P[:W * K - 1]), dict(d_first=d_first[:2]),
                   dict(d_count=d_count[:2]), dict(d_first=d_first.to(torch.int32)),
                   dict(d_count=d_count.to(torch.int64)), dict(d_count=d_count.cpu()),
                   dict(d_hits=g_hits[:S * cap * HIT - 1]), dict(d_hits=None),
                   dict(d_payload=g_pay[:S * cap * N - 1]), dict(d_packed=g_pak[:S * cap * N * 3 // 8 - 1]),
                   dict(d_results=g_res[:S * RES_BYTES - 1]), dict(d_results=g_res.to(torch.int16)),
                   dict(d_work=g_work[:-1])):
            a = dict(base)
            a.update(kw)
            with pytest.raises(A.DemodError) as e:
                d.frames_segments_async(a["d_sym"], a["d_mag"], W, a["d_first"], a["d_count"], S, good, 0, N,
                                        a["d_hits"], a["d_payload"], a["d_packed"], cap, a["d_results"],
                                        a["d_work"])
            assert e.value.code == A.DEMOD_BAD_ARG
        for chk in (chk_hits, chk_pay, chk_pak, chk_res, chk_work):
            chk(written=False)
        for t in (g_hits, g_pay, g_pak, g_res, g_work):
            assert bool((t == 0xFF).all()), "a refused call wrote"
        # and the same call, legal, runs; so does a count-only one
        assert call() == A.DEMOD_OK
        torch.cuda.synchronize()
        raw = g_res.cpu().numpy().tobytes()
        first_run = [parse(A, raw[s * RES_BYTES:(s + 1) * RES_BYTES]) for s in range(S)]
        assert [r["per_phase"] for r in first_run] == [250, 500, 274]
        g_res.fill_(0xFF)
        assert call(hits=None, pay=None, pak=None, cap=0) == A.DEMOD_OK
        torch.cuda.synchronize()
        raw = g_res.cpu().numpy().tobytes()
        counted = [parse(A, raw[s * RES_BYTES:(s + 1) * RES_BYTES]) for s in range(S)]
        assert [r["n_hits"] for r in counted] == [r["n_hits"] for r in first_run]
        assert not any(r["n_written"] for r in counted)
        # n_windows below R is legal here: every segment is short
        assert call(W=3) == A.DEMOD_OK
        torch.cuda.synchronize()
        raw = g_res.cpu().numpy().tobytes()
        for s in range(S):
            assert raw[s * RES_BYTES:(s + 1) * RES_BYTES] == result_bytes(A, FS.short_result(4))
        # the longest legal frame, (L + N) R = 2^31 - 4: nothing is complete
        assert call(N=2 ** 29 - 9, cap=0, hits=None, pay=None, pak=None) == A.DEMOD_OK
        torch.cuda.synchronize()
        raw = g_res.cpu().numpy().tobytes()
        assert not any(parse(A, raw[s * RES_BYTES:(s + 1) * RES_BYTES])["n_hits"] for s in range(S))
    finally:
        for dd in others + [d]:
            dd.close()


# ---- 9. end to end -------------------------------------------------------------

DETECTORS = {"slide": (F.FSK2, "METHOD_AUTO"), "fold_slide": (F.FSK8, "METHOD_AUTO"),
             "fft": (F.FSK2, "METHOD_FFT")}
TAUS = (0, 64, 100, 192, 256, 320, 448, 512, 576, 700, 768, 960)      # none half-way between two phases


@functools.lru_cache(maxsize=None)
def recordings(freqs):
    """Twelve frame_stream recordings, each at its own tau and cut to its own
    length (the last frame stays whole), with the single-stream reference of
    each on the oracle's double powers."""
    from oracle import oracle as O
    out = []
    for i, tau in enumerate(TAUS):
        x, word, payloads, windows = F.frame_stream(freqs, tau)
        x = x[:len(x) - 29 * i]
        sym, P = O.goertzel(x, freqs, 1024, 256)
        out.append((x, word, payloads, windows, F.frames(sym, P, 4, word, 1, F.FRAME_N)))
    return out


@pytest.mark.parametrize("name", sorted(DETECTORS))
def test_many_recordings(A, torch, name):
    """Twelve recordings laid out by segments_layout as one batch, through one
    sliding detector, from host and device PCM via Demodulator.frames_segments:
    each one's phase, windows, payloads and packed bytes equal its own
    single-stream reference and the planted truth."""
    freqs, method = DETECTORS[name]
    n, hop, Rn = 1024, 256, 4
    bits = F.bits_per_symbol(len(freqs))
    recs = recordings(freqs)
    word = recs[0][1]
    cfg = A.make_cfg(n=n, hop=hop, freqs=freqs, method=getattr(A, method))
    first, count, Wb = A.segments_layout(cfg, [len(r[0]) for r in recs])
    batch = np.zeros((Wb - 1) * hop + n, np.int16)
    for r, f in zip(recs, first):
        batch[int(f) * hop:int(f) * hop + len(r[0])] = r[0]
    with A.Demodulator(cfg) as d:
        assert d.method == {"slide": A.METHOD_GOERTZEL, "fold_slide": A.METHOD_FOLDED, "fft": A.METHOD_FFT}[name]
        for pcm in (batch, torch.from_numpy(batch).cuda()):
            got = d.frames_segments(pcm, first, count, word, max_errors=1, frame_symbols=F.FRAME_N)
            assert len(got) == len(recs)
            phases = set()
            for s, ((hits, pay, pak, res), (x, _, payloads, windows, ref)) in enumerate(zip(got, recs)):
                r_hits, r_pay, r_pak, r_res = ref
                # the fixture's condition, on the reference alone
                assert r_hits["window"].tolist() == windows.tolist() and np.array_equal(r_pay, payloads)
                assert r_res["phase"] == ((TAUS[s] + 128) // 256) % Rn and r_res["tail_window"] == -1
                assert res["phase"] == r_res["phase"] and res["per_phase"] == r_res["per_phase"] == count[s] // Rn
                assert res["n_hits"] == res["n_written"] == F.FRAME_COUNT and res["tail_window"] == -1
                assert hits.tobytes() == r_hits.tobytes()
                assert np.array_equal(pay, payloads) and np.array_equal(pak, F.pack(payloads, bits))
                err = np.abs(res["metric"] - r_res["metric"])
                assert (err <= (G.MAG_TOL + r_res["per_phase"] * 2.0 ** -52) * r_res["metric"]).all()
                phases.add(res["phase"])
            assert phases == set(range(Rn))
        # a short max_frames cuts the lists, not the counts; payload alone
        got = d.frames_segments(batch, first, count, word, max_errors=1, frame_symbols=F.FRAME_N,
                                max_frames=2, packed=False)
        for (hits, pay, pak, res), rec in zip(got, recs):
            assert res["n_hits"] == F.FRAME_COUNT and res["n_written"] == 2 and pak is None
            assert hits.tobytes() == rec[4][0][:2].tobytes() and np.array_equal(pay, rec[2][:2])


@functools.lru_cache(maxsize=None)
def slip_reference(freqs):
    from oracle import oracle as O
    x, word, payloads, cut, rel = FS.slip_stream(freqs)
    sym, P = O.goertzel(x, freqs, 1024, 256)
    return x, word, payloads, cut, rel, sym, P


@pytest.mark.parametrize("name", sorted(DETECTORS))
def test_slip_end_to_end(A, torch, name):
    """n / 2 samples deleted two symbols before the third of five frames: as
    two segments split at the slip the detectors give all five frames with
    exact payloads (phases 0 and 2), where the whole-batch call returns fewer."""
    freqs, method = DETECTORS[name]
    Rn = 4
    x, word, payloads, cut, rel, sym, P = slip_reference(freqs)
    W = len(sym)
    first, count = [0, cut], [cut, W - cut]
    want = FS.frames_segments(sym, P, Rn, first, count, word, 1, F.FRAME_N)
    assert F.frames(sym, P, Rn, word, 1, F.FRAME_N)[3]["n_hits"] < F.FRAME_COUNT
    with A.Demodulator(n=1024, hop=256, freqs=freqs, method=getattr(A, method)) as d:
        whole = d.frames(x, word, max_errors=1, frame_symbols=F.FRAME_N)
        print(f"{name}: whole batch phase {whole[3]['phase']} hits {whole[0]['window'].tolist()}")
        assert whole[3]["n_hits"] < F.FRAME_COUNT
        for pcm in (x, torch.from_numpy(x).cuda()):
            got = d.frames_segments(pcm, first, count, word, max_errors=1, frame_symbols=F.FRAME_N)
            assert [g[3]["phase"] for g in got] == [0, 2]
            assert got[0][0]["window"].tolist() + got[1][0]["window"].tolist() == rel
            assert np.array_equal(np.concatenate([got[0][1], got[1][1]]), payloads)
            assert np.array_equal(np.concatenate([got[0][2], got[1][2]]),
                                  F.pack(payloads, F.bits_per_symbol(len(freqs))))
            for g, r in zip(got, want):
                assert g[0].tobytes() == r[0].tobytes() and np.array_equal(g[1], r[1])
                assert g[3]["n_hits"] == r[3]["n_hits"] and g[3]["tail_window"] == r[3]["tail_window"] == -1


# ---- 10. capture and replay ------------------------------------------------------

def test_capture_and_replay(A, torch):
    """demod_batch_async + demod_frames_segments_async in one graph on a side
    stream: replayed on new PCM, and again after d_first / d_count were
    rewritten in place with another segmentation. Each replay's bytes are the
    eager bytes for that content and those tables, and the reference's rows."""
    freqs, N, cap, Rn, S = F.FSK2, F.FRAME_N, 6, 4, 3
    from oracle import oracle as O
    refs = []
    for tau, drop in ((256, ()), (576, (1, 3))):
        x = F.frame_stream(freqs, tau, drop=drop)[0]
        refs.append((x,) + tuple(O.goertzel(x, freqs, 1024, 256)))
    word = F.frame_stream(freqs, 256)[1]
    W = min(len(r[1]) for r in refs)
    need = (W - 1) * 256 + 1024
    segmentations = [([0, W // 2 // Rn * Rn, 0], [W // 2 // Rn * Rn, W - W // 2 // Rn * Rn, 0]),
                     ([W - 900, 7, 0], [900, 2, W])]
    with A.Demodulator(n=1024, hop=256, freqs=freqs) as d:
        d_pcm = torch.zeros(need, dtype=torch.int16, device="cuda")
        d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
        d_mag = torch.empty(W * d.k, dtype=torch.float32, device="cuda")
        outs = [torch.empty(nb, dtype=torch.uint8, device="cuda")
                for nb in (S * cap * HIT, S * cap * N, S * cap * N // 8, S * RES_BYTES)]
        d_work = torch.empty(A.frames_segments_workspace_size(d.cfg, S, W), dtype=torch.uint8, device="cuda")
        d_first, d_count = tables(torch, *segmentations[0])

        def step(stream):
            d.batch_async(d_pcm, W, d_sym, d_mag, stream=stream)
            d.frames_segments_async(d_sym, d_mag, W, d_first, d_count, S, word, 1, N, outs[0], outs[1],
                                    outs[2], cap, outs[3], d_work, stream=stream)

        def load(i, seg):
            nf, nc = tables(torch, *segmentations[seg])
            d_first.copy_(nf)                                    # in place: the graph holds the pointers
            d_count.copy_(nc)
            d_pcm.copy_(torch.from_numpy(refs[i][0][:need]))
            for t in outs:
                t.fill_(0xFF)
            d_work.fill_(0xFF)

        def results():
            torch.cuda.synchronize()
            return [t.cpu().numpy().tobytes() for t in outs]

        side = torch.cuda.Stream()
        eager = {}
        with torch.cuda.stream(side):
            for seg in range(2):
                for i in range(2):                               # eager calls of the shape first
                    load(i, seg)
                    step(side.cuda_stream)
                    side.synchronize()
                    eager[i, seg] = results()
        load(0, 0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step(torch.cuda.current_stream().cuda_stream)
        for rep in range(2):
            for seg in range(2):
                for i in range(2):
                    load(i, seg)
                    torch.cuda.synchronize()
                    g.replay()
                    assert results() == eager[i, seg], (rep, seg, i)
        hits_seen = 0
        for (i, seg), got in eager.items():
            first, count = segmentations[seg]
            sym, P = refs[i][1][:W], refs[i][2][:W]
            want = FS.frames_segments(sym, P, Rn, first, count, word, 1, N)
            hits = np.frombuffer(got[0], F.HIT_DTYPE).reshape(S, cap)
            pay = np.frombuffer(got[1], np.uint8).reshape(S, cap, N)
            pak = np.frombuffer(got[2], np.uint8).reshape(S, cap, N // 8)
            for s, (r_hits, r_pay, r_pak, r_res) in enumerate(want):
                res = parse(A, got[3][s * RES_BYTES:(s + 1) * RES_BYTES])
                for f in ("phases", "phase", "per_phase", "n_hits", "n_written", "tail_window", "tail_errors"):
                    assert res[f] == r_res[f], (i, seg, s, f)
                n = r_res["n_hits"]
                assert n <= cap and hits[s, :n].tobytes() == r_hits.tobytes()
                assert (hits[s, n:].view(np.uint8) == 0xFF).all()
                assert np.array_equal(pay[s, :n], r_pay) and np.array_equal(pak[s, :n], r_pak)
                hits_seen += n
        assert hits_seen >= 12
