"""Segmented acquisition on the GPU (acquire_segments.hip) against
tests/acquire_segments_ref.py: S segments of one batch, each acquired as a
batch of its own, in one call.

Kernel level: test-made sym / P on the device, R in {1, 4, 64} x K in {1, 2,
16}, segment lengths around R and around the tile T = ACQUIRE_TILE.

  metric   |M - M_ref| <= J 2^-52 M_ref per phase: M_ref is the correctly
           rounded sum (math.fsum) and any order of summing J non-negative
           doubles is within (J - 1) 2^-53 (1 + o(1)) of the exact sum.
  every integer field and every output byte: equal to the reference's.

Segments of 66 tiles take the finaliser's workgroup path; DEMOD_MAX_SEGMENTS
short segments take the plan's rounds and the scan's loop to their ends.

End to end: the slip scenario of tests/test_acquire_segments_cpu.py through the
detectors, twelve recordings in one batch, and a captured graph replayed after
its tables were rewritten in place.
"""
import functools

import numpy as np
import pytest

import acquire_ref as R
import acquire_segments_ref as SR
import guards as G
from acquire_ref import make_inputs, plant
from guards import MAG_TOL
from gpu_support import (ACQUIRE_INT_FIELDS as INT_FIELDS, EPS, check_acquire as check, handle_fixture, parse_acquire
                         as parse, phased, tables, tones_375, torch)  # noqa: F401

pytestmark = pytest.mark.gpu

# (n, hop) of a handle with R = n / hop phases
SHAPE_OF_R = {1: (1024, 1024), 4: (1024, 256), 64: (512, 8)}
RS = sorted(SHAPE_OF_R)
KS = (1, 2, 16)
RES_BYTES = R.RESULT_DTYPE.itemsize
LEAD = 4096          # guard bytes per side (a multiple of 8: d_results and d_work stay aligned)


# handle(R, K): one Demodulator per (R, K), closed with the module.
handle = handle_fixture(lambda A, Rn, K: phased(A, SHAPE_OF_R, Rn, tones_375(K)))


class Runner:
    """Device buffers of one (handle, batch): run(first, count, ...) puts d_out,
    d_results and d_work between poisoned guards and checks them."""

    def __init__(self, A, torch, d, sym, P):
        self.A, self.torch, self.d = A, torch, d
        self.Wb = len(sym)
        self.d_sym = torch.from_numpy(np.ascontiguousarray(sym)).cuda()
        self.d_P = torch.from_numpy(np.ascontiguousarray(P)).cuda()

    def run(self, first, count, sync=None, max_errors=0, cap=0, stream=0, sym=None, poison=0xFF,
            work_windows=None, nan_work=False):
        A, torch = self.A, self.torch
        S = len(first)
        if sym is not None:
            self.d_sym.copy_(torch.from_numpy(sym))
        d_first, d_count = tables(torch, first, count)
        g_out, chk_out = (G.guarded(torch, S * cap, torch.uint8, LEAD + 1, LEAD, 0xFF) if cap
                          else (None, lambda written: None))
        g_res, chk_res = G.guarded(torch, S * RES_BYTES, torch.uint8, LEAD, LEAD, poison)
        wb = A.acquire_segments_workspace_size(self.d.cfg, S, self.Wb if work_windows is None
                                               else work_windows)
        g_work, chk_work = G.guarded(torch, wb, torch.uint8, LEAD, LEAD, poison)
        if nan_work:
            g_work.view(torch.int32).fill_(G.F32_POISON)
        self.d.acquire_segments_async(self.d_sym, self.d_P, self.Wb, d_first, d_count, S, sync,
                                      max_errors, g_out, g_res, g_work, stream=stream)
        chk_out(written=False)
        chk_res(written=False)
        chk_work(written=False)
        raw = g_res.cpu().numpy().tobytes()
        raws = [raw[s * RES_BYTES:(s + 1) * RES_BYTES] for s in range(S)]
        out = g_out.cpu().numpy().reshape(S, cap) if cap else np.zeros((S, 0), np.uint8)
        return out, [parse(A, r) for r in raws], raws


def check_all(got, want, cap, metric=True):
    out, res, _ = got
    assert len(res) == len(want)
    for s, (ref_out, ref) in enumerate(want):
        check(res[s], out[s], ref_out, ref, cap, metric)


def layout(counts, gap):
    first, at = [], 0
    for c in counts:
        first.append(at)
        at += c + gap
    return first, max(at - gap, 1)


def fill(Wb, K, Rn, first, count, seed, flat=False, gap_poison=False):
    """A batch whose segments hold make_inputs contents of their own (phase
    (s + 1) % R boosted, relative to the segment) and whose other windows are
    random, or (gap_poison) sym 0 with P alternately NaN and 3e38."""
    sym, P = make_inputs(Wb, K, Rn, seed, flat=flat)
    if gap_poison:
        sym[:] = 0
        P[0::2] = np.float32(np.nan)
        P[1::2] = np.float32(3e38)
    for s, (f, c) in enumerate(zip(first, count)):
        if c:
            sym[f:f + c], P[f:f + c] = make_inputs(c, K, Rn, seed + 100 + s, (s + 1) % Rn, flat)
    return sym, P


def whole_batch_agrees(A, torch, d, run, first, count, sync, max_errors, res):
    """demod_acquire_async on each slice of at least R windows (clamped as the
    kernels clamp): the same integer fields as the segmented call's res."""
    Rn = d.n // d.hop
    d_work = torch.empty(A.acquire_workspace_size(d.cfg), dtype=torch.uint8, device="cuda")
    d_res = torch.empty(RES_BYTES, dtype=torch.uint8, device="cuda")
    for s, (f, c) in enumerate(zip(first, count)):
        f, c = SR.clamp(f, c, run.Wb)
        if c < Rn or res[s]["per_phase"] == 0:
            continue
        d.acquire_async(run.d_sym[f:f + c], run.d_P[f:f + c].reshape(-1), c, sync, max_errors, None,
                        d_res, d_work)
        torch.cuda.synchronize()
        one = parse(A, d_res.cpu().numpy().tobytes())
        for fld in INT_FIELDS:
            assert one[fld] == res[s][fld], (s, fld, one[fld], res[s][fld])


# ---- 1. equivalence ----------------------------------------------------------

@pytest.mark.parametrize("Rn", RS)
@pytest.mark.parametrize("K", KS)
def test_equivalence(A, torch, handle, Rn, K):
    """Nine segments around R and around the tile, shuffled; touching, with gaps
    of R - 1 windows, and with `first` reversed: every field and byte equals the
    reference's, and the integer fields equal demod_acquire_async's on the slice."""
    T = A.ACQUIRE_TILE
    d = handle(Rn, K)
    counts = [0, Rn - 1, Rn, Rn + 1, T - 1, T, T + 1, 2 * T + 5, 3]
    counts = [counts[i] for i in np.random.default_rng(Rn * 31 + K).permutation(len(counts))]
    word = ((np.arange(5) * 3 + 1) % K).astype(np.uint8)
    cap = (2 * T + 5) // Rn + 2
    found = 0
    for variant, gap in (("touching", 0), ("gaps", Rn - 1), ("reversed", Rn - 1)):
        first, Wb = layout(counts, gap)
        count = list(counts)
        if variant == "reversed":      # the same slices listed from the last to the first
            first, count = first[::-1], count[::-1]
        sym, P = fill(Wb, K, Rn, first, count, 7 * Rn + K)
        # a word of 5 on each segment's boosted phase, one byte >= K in it: one error
        for s, (f, c) in enumerate(zip(first, count)):
            if c >= 12 * Rn:
                w0 = f + (s + 1) % Rn + (c // Rn - 6) // 2 * Rn
                sym[w0:w0 + 5 * Rn:Rn] = word
                sym[w0 + 2 * Rn] = 0x80
        run = Runner(A, torch, d, sym, P)
        for sync, me in ((None, 0), (word, 1)):
            want = SR.acquire_segments(sym, P, Rn, first, count, () if sync is None else sync, me)
            for _, ref in want:
                assert Rn == 1 or ref["per_phase"] == 0 or R.margin(ref["metric"]) > 1e-6
            got = run.run(first, count, sync, me, cap)
            check_all(got, want, cap)
            whole_batch_agrees(A, torch, d, run, first, count, sync, me, got[1])
        # (the planted symbols pick other powers: a phase may move off its word)
        found += sum(ref["sync_window"] >= 0 for _, ref in want)
    assert found >= 3      # of 12 planted (R = 64, K = 16 keeps 3: 16 windows a phase, 5 replanted)


# ---- 2. isolation ------------------------------------------------------------

@pytest.mark.parametrize("Rn,K,max_errors,gap", [(1, 2, 0, 0), (1, 16, 1, 2), (4, 16, 2, 0), (4, 2, 1, 3),
                                                 (64, 2, 3, 0), (64, 16, 0, 63)])
def test_isolation(A, torch, handle, Rn, K, max_errors, gap):
    """A sync word lying across a segment boundary is not found, whichever way
    it is split; at the last legal start of a segment it is. The windows
    between segments (gap > 0) are NaN / 3e38 powers and never read."""
    T, L = A.ACQUIRE_TILE, 24
    rng = np.random.default_rng(Rn * 5 + K)
    # segments that end inside a tile, on a tile's end and one window past it
    # (each with at least L windows on a phase)
    big = T if T // Rn >= L + 2 else 2 * T
    counts = [big + 5 * Rn, big, max(T // 2, (L + 4) * Rn) + 1, (L + 2) * Rn]
    first, Wb = layout(counts, gap)
    sym, P = fill(Wb, K, Rn, first, counts, 40 + Rn + K, flat=True, gap_poison=gap > 0)
    word = rng.integers(0, K, L).astype(np.uint8)
    d = handle(Rn, K)
    run = Runner(A, torch, d, sym, P)
    cap = max(counts) // Rn + 1
    base = SR.acquire_segments(sym, P, Rn, first, counts, word, max_errors)
    phase = [ref["phase"] for _, ref in base]
    assert all(ref["sync_window"] == -1 for _, ref in base)      # no match to begin with
    assert all(Rn == 1 or R.margin(ref["metric"]) > 1e-6 for _, ref in base)
    check_all(run.run(first, counts, word, max_errors, cap), base, cap)

    def go(s2, metric=True):      # (the plants are symbols < K on flat powers: the metric stays)
        want = SR.acquire_segments(s2, P, Rn, first, counts, word, max_errors)
        check_all(run.run(first, counts, word, max_errors, cap, sym=s2), want, cap, metric)
        return [ref["sync_window"] for _, ref in want]

    def phase_windows(s):
        return first[s] + np.arange(phase[s], counts[s], Rn)

    # the word across each boundary: its first i symbols end segment s, the rest start s + 1
    for s in range(len(counts) - 1):
        tail, head = phase_windows(s), phase_windows(s + 1)
        for i in range(1, L):
            s2 = sym.copy()
            s2[tail[len(tail) - i:]] = word[:i]
            s2[head[:L - i]] = word[i:]
            assert go(s2) == [-1] * len(counts), (s, i)
    # the last legal start of each segment: found; with max_errors mismatches: found, one more: not
    for s in range(len(counts)):
        last = phase_windows(s)[-L] - first[s]
        for n_bad in (0, max_errors, max_errors + 1):
            if K == 1 and n_bad:
                continue
            s2 = plant(sym, Rn, first[s] + last, word, n_bad, K, rng)
            found = go(s2)
            assert found == [(last if j == s and n_bad <= max_errors else -1) for j in range(len(counts))]
        # one phase step later the word no longer fits: the symbols that do fit are not a match
        s2 = sym.copy()
        s2[phase_windows(s)[-(L - 1):]] = word[:L - 1]
        assert go(s2)[s] == -1


# ---- 3. position independence ------------------------------------------------

@pytest.mark.parametrize("Rn,K", [(4, 2), (64, 16), (1, 1)])
def test_position_independence(A, torch, handle, Rn, K):
    """One segment's contents at three places, in slots 0, 1 and S - 1, beside
    different neighbours, S in {1, 3, 1025}, and on a second stream: the same
    result bytes and the same output row every time."""
    T = A.ACQUIRE_TILE
    c0 = 2 * T + 37 * Rn + 3
    seg_sym, seg_P = make_inputs(c0, K, Rn, 99 + Rn, boost=Rn // 2)
    # 14 decades of powers: the largest few decide the phase, not the 1.5
    ph = int(np.argmax(R.phase_metric(seg_sym, seg_P, Rn)[0]))
    word = seg_sym[ph + 10 * Rn:ph + 34 * Rn:Rn].copy()
    ref_out, ref = R.acquire(seg_sym, seg_P, Rn, word, 2)
    assert ref["sync_window"] >= 0
    cap = c0 // Rn + 1
    d = handle(Rn, K)
    seen = []
    side = torch.cuda.Stream()
    for S, slots in ((1, (0,)), (3, (0, 1, 2)), (1025, (0, 1, 1024))):
        for slot in slots:
            rng = np.random.default_rng(1000 * S + slot)
            counts = [int(v) for v in rng.integers(0, 40, S)]
            counts[slot] = c0
            first, Wb = layout(counts, int(rng.integers(0, 5)))
            lead = int(rng.integers(0, 3000))         # the batch starts with windows of no segment
            first = [f + lead for f in first]
            Wb += lead
            sym, P = fill(Wb, K, Rn, first, counts, S + slot)
            sym[first[slot]:first[slot] + c0] = seg_sym
            P[first[slot]:first[slot] + c0] = seg_P
            run = Runner(A, torch, d, sym, P)
            out, res, raws = run.run(first, counts, word, 2, cap)
            check(res[slot], out[slot], ref_out, ref, cap)
            seen.append((raws[slot], out[slot].tobytes()))
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                out2, _, raws2 = run.run(first, counts, word, 2, cap, stream=side.cuda_stream)
            assert raws2 == raws and np.array_equal(out2, out)
            if S == 3:      # the neighbours, too, equal the reference
                check_all((out, res, raws), SR.acquire_segments(sym, P, Rn, first, counts, word, 2), cap)
    assert len(seen) == 7 and all(v == seen[0] for v in seen)


# ---- 4. clamping and the tile budget -----------------------------------------

@pytest.mark.parametrize("Rn,K", [(1, 16), (4, 1), (4, 2), (64, 2)])
def test_clamp_budget_and_guards(A, torch, handle, Rn, K):
    """Tables no host has checked: first >= Wb, first + count > Wb, count =
    0xFFFFFFFF, and overlapping segments past the workspace's tile budget;
    d_work poisoned with 0xFF and with NaN bits; cap 0 without d_out."""
    T = A.ACQUIRE_TILE
    Wb = 3 * T + 100
    first = [0, Wb + 5, Wb - Rn - 1, 0, 0, 5, T, 0, 1 << 40, Wb, 0]
    count = [0xFFFFFFFF, 10, 100, Wb, Wb, Rn, 2 * T + 1, min(2, Rn), 7, 0xFFFFFFFF, Wb]
    S = len(first)
    budget = SR.budget_for(S, Wb)
    assert budget == 4 + S
    sym, P = make_inputs(Wb, K, Rn, 17 + Rn, boost=Rn - 1)
    word = sym[Rn - 1 + 8 * Rn:Rn - 1 + 14 * Rn:Rn].copy()
    want = SR.acquire_segments(sym, P, Rn, first, count, word, 1, budget=budget)
    # what the rules give, by the definitions alone: 4 + 1 + 4 + 4 + 1 = 14 tiles fit the 15,
    # the 3 of segment 6 do not, and nothing after it does
    assert [ref["per_phase"] > 0 for _, ref in want] == [True, False] + [True] * 4 + [False] * 5
    assert want[6][1]["first_window"] == 2 * T + 1 and want[10][1]["first_window"] == Wb
    assert want[7][1]["first_window"] == min(2, Rn)
    assert want[1][1]["first_window"] == 0 and want[8][1]["first_window"] == 0
    run = Runner(A, torch, handle(Rn, K), sym, P)
    cap = Wb // Rn + 3
    raws = []
    for poison, nan_work in ((0xFF, False), (0x5A, False), (0xFF, True)):
        got = run.run(first, count, word, 1, cap, poison=poison, nan_work=nan_work)
        check_all(got, want, cap)
        raws.append(got[2])
    assert raws[0] == raws[1] == raws[2]          # every byte of d_results is written
    # a short cap cuts the rows, not the counts; cap 0 takes no d_out at all
    got = run.run(first, count, word, 1, 3)
    check_all(got, want, 3)
    got0 = run.run(first, count, word, 1, 0)
    check_all(got0, want, 0)
    # a workspace sized for overlapping callers holds them all
    full = SR.acquire_segments(sym, P, Rn, first, count, word, 1)
    wide = run.run(first, count, word, 1, cap, work_windows=4 * Wb)
    check_all(wide, full, cap)
    assert full[10][1]["per_phase"] == Wb // Rn and full[6][1]["per_phase"] == (2 * T + 1) // Rn
    assert wide[2][0] == raws[0][0]               # and segment 0 does not notice


# ---- 5. refusals -------------------------------------------------------------

def test_refusals(A, torch):
    """Every DEMOD_BAD_ARG case returns without a launch: results, rows and
    workspace stay poison."""
    lib = A.load_library()
    K, W, S, cap = 8, 4096, 3, 64
    d = A.Demodulator(n=1024, hop=256, freqs=tuple(1500.0 + 375.0 * i for i in range(K)))
    others = [A.Demodulator(n=1024, hop=384, freqs=(1500.0, 3000.0)),
              A.Demodulator(n=1024, hop=8, freqs=(1500.0, 3000.0))]
    try:
        sym, P = make_inputs(W, K, 4, 1)
        d_sym, d_P = torch.from_numpy(sym).cuda(), torch.from_numpy(P).cuda()
        d_first, d_count = tables(torch, [0, 1000, 3000], [1000, 2000, 1096])
        wb = A.acquire_segments_workspace_size(d.cfg, S, W)
        g_out, chk_out = G.guarded(torch, S * cap, torch.uint8, LEAD, LEAD, 0xFF)
        g_res, chk_res = G.guarded(torch, S * RES_BYTES, torch.uint8, LEAD, LEAD, 0xFF)
        g_work, chk_work = G.guarded(torch, wb, torch.uint8, LEAD, LEAD, 0xFF)
        good = np.arange(8, dtype=np.uint8)
        bad_sym = np.array([0, K], np.uint8)
        long_word = np.zeros(65, np.uint8)
        ps, pm, pf, pc, po, pr, pw = (t.data_ptr() for t in (d_sym, d_P, d_first, d_count, g_out,
                                                             g_res, g_work))
        sp = good.ctypes.data
        ok = dict(h=d._h, sym=ps, mag=pm, W=W, first=pf, count=pc, S=S, sync=sp, L=8, me=0, out=po,
                  cap=cap, res=pr, work=pw, wb=wb)

        def call(**kw):
            a = dict(ok)
            a.update(kw)
            return lib.demod_acquire_segments_async(a["h"], a["sym"], a["mag"], a["W"], a["first"],
                                                    a["count"], a["S"], a["sync"], a["L"], a["me"],
                                                    a["out"], a["cap"], a["res"], a["work"], a["wb"],
                                                    None)

        cases = [
            ("NULL handle", dict(h=None)),
            ("W >= 2^31", dict(W=1 << 31)),
            ("sync_len > 64", dict(sync=long_word.ctypes.data, L=65)),
            ("sync symbol >= K", dict(sync=bad_sym.ctypes.data, L=2)),
            ("max_errors >= sync_len", dict(me=8)),
            ("NULL sync with sync_len", dict(sync=None)),
            ("NULL d_symbols", dict(sym=None)),
            ("NULL d_mags", dict(mag=None)),
            ("NULL d_results", dict(res=None)),
            ("NULL d_work", dict(work=None)),
            ("NULL d_out with cap", dict(out=None)),
            ("NULL d_first", dict(first=None)),
            ("NULL d_count", dict(count=None)),
            ("n_segments == 0", dict(S=0)),
            ("n_segments > DEMOD_MAX_SEGMENTS", dict(S=A.DEMOD_MAX_SEGMENTS + 1, wb=1 << 40)),
            ("work_bytes one short", dict(wb=wb - 1)),
            ("work_bytes 0", dict(wb=0)),
            ("misaligned d_results", dict(res=pr + 4)),
            ("misaligned d_work", dict(work=pw + 4)),
            ("misaligned d_first", dict(first=pf + 4)),
            ("misaligned d_count", dict(count=pc + 2)),
            ("n % hop != 0", dict(h=others[0]._h, sync=None, L=0)),
            ("R > 64", dict(h=others[1]._h, sync=None, L=0)),
        ]
        for what, kw in cases:
            assert call(**kw) == A.DEMOD_BAD_ARG, what
        # the synchronous call checks its host tables before the detector runs
        x = np.zeros(16 * 1024, np.int16)
        for f, c in [([0, 70], [20, 2]), ([0, 30], [20, 32]), ([62], [4]), ([0], [3])]:
            with pytest.raises(A.DemodError) as e:
                d.acquire_segments(x, f, c)                         # 61 windows, R = 4
            assert e.value.code == A.DEMOD_BAD_ARG, (f, c)
        for dd in others:
            with pytest.raises(A.DemodError) as e:
                dd.acquire_segments(x, [0], [8])
            assert e.value.code == A.DEMOD_BAD_ARG
        # the Python mirror's own checks (before any pointer reaches the library)
        base = dict(d_sym=d_sym, d_mag=d_P, d_first=d_first, d_count=d_count, d_results=g_res,
                    d_work=g_work)
        for kw in (dict(d_sym=d_sym[:W - 1]), dict(d_first=d_first[:2]), dict(d_count=d_count[:2]),
                   dict(d_first=d_first.to(torch.int32)), dict(d_count=d_count.cpu()),
                   dict(d_results=g_res[:S * RES_BYTES - 1]), dict(d_work=g_work[:-1])):
            a = dict(base)
            a.update(kw)
            with pytest.raises(A.DemodError) as e:
                d.acquire_segments_async(a["d_sym"], a["d_mag"], W, a["d_first"], a["d_count"], S, good,
                                         0, g_out, a["d_results"], a["d_work"])
            assert e.value.code == A.DEMOD_BAD_ARG
        chk_out(written=False)
        chk_res(written=False)
        chk_work(written=False)
        for t in (g_out, g_res, g_work):
            assert bool((t == 0xFF).all()), "a refused call wrote"
        # and the same call, legal, runs; n_windows below R is legal here: every segment is short
        assert call() == A.DEMOD_OK
        torch.cuda.synchronize()
        assert parse(A, g_res.cpu().numpy().tobytes()[:RES_BYTES])["per_phase"] == 250
        assert call(W=3, sync=None, L=0) == A.DEMOD_OK
        torch.cuda.synchronize()
        raw = g_res.cpu().numpy().tobytes()
        got = [parse(A, raw[s * RES_BYTES:(s + 1) * RES_BYTES]) for s in range(S)]
        assert [r["first_window"] for r in got] == [3, 0, 0] and not any(r["per_phase"] for r in got)
    finally:
        for dd in others + [d]:
            dd.close()


# ---- 6. end to end: the slip -------------------------------------------------

@functools.lru_cache(maxsize=None)
def slip_reference(name, drop):
    """(x, truth, cut, phase2, oracle sym, oracle P): computed once per case and drop."""
    from oracle import oracle as O
    freqs, n, hop = R.CASES[name][:3]
    x, truth, cut, phase2 = SR.slip_stream(O, name, drop)
    sym, P = O.goertzel(x, freqs, n, hop)
    return x, truth, cut, phase2, sym, P


@pytest.mark.parametrize("name,method", [("A", "AUTO"), ("D", "AUTO"), ("A", "FFT")])
def test_slip_end_to_end(A, torch, name, method):
    """A stream that loses hop, 2 hop and 3 hop samples in its middle, through
    the real detectors (A: the segment-shared plain bank, D: the carried fold,
    A again through the FFT): two segments split at the slip give each side's
    phase and the transmitted symbols; the whole batch has one phase for both.

    As one batch the phase margin collapses and the windows after the slip hold
    n - drop samples of symbol i and drop samples of symbol i + 1: from drop =
    n / 2 on, Demodulator.acquire's stream no longer reproduces the truth (on
    the oracle: 19 .. 72 symbols wrong); at drop = hop = n / 4 it still does,
    on three quarters of a window (0 wrong on the oracle), so the whole-batch
    failure is asserted for 2 drop >= n and printed for drop = hop."""
    freqs, n, hop, ns = R.CASES[name][:4]
    Rn = n // hop
    with A.Demodulator(n=n, hop=hop, freqs=freqs, method=getattr(A, "METHOD_" + method)) as d:
        if method == "AUTO":
            assert d.slide_windows > 0
        for drop in SR.slip_drops(n, hop):
            x, truth, cut, phase2, sym, P = slip_reference(name, drop)
            W = len(sym)
            first, count = [0, cut], [cut, W - cut]
            want = SR.acquire_segments(sym, P, Rn, first, count)
            for src in (x, torch.from_numpy(x).cuda()):
                out, res = d.acquire_segments(src, first, count)
                assert out.shape == (2, max(count) // Rn + 1)
                for s, (ref_out, ref) in enumerate(want):
                    Mr = ref["metric"]
                    assert R.margin(Mr) > 4e-5                     # the reference's margin, first
                    for f in INT_FIELDS:
                        assert res[s][f] == ref[f], (s, f)
                    err = np.abs(res[s]["metric"] - Mr)
                    print(f"case {name} {method} drop {drop} segment {s}: phase {res[s]['phase']} "
                          f"max |M - M_ref| / M_ref {float((err / Mr).max()):.3e}")
                    assert (err <= MAG_TOL * Mr + ref["per_phase"] * EPS * Mr).all()
                    nw = res[s]["n_written"]
                    assert nw == ref["n_out"] and np.array_equal(out[s, :nw], ref_out)
                    assert (out[s, nw:] == 0xFF).all()
                assert res[0]["phase"] == 0 and res[1]["phase"] == phase2
                after = truth[ns // 2 + 1:]
                got = out[1, :res[1]["n_written"]]
                assert np.array_equal(got, after[:len(got)]) and len(after) - len(got) <= 1
                assert np.array_equal(out[0, :res[0]["n_written"]], truth[:ns // 2])
            whole_out, whole = d.acquire(x)
            bad = SR.whole_batch_misreads(whole_out, truth, ns)
            print(f"case {name} {method} drop {drop}: whole batch phase {whole['phase']} margin "
                  f"{R.margin(whole['metric']):.4f}, {bad} symbols after the slip misread")
            assert whole["phase"] != phase2
            assert bad > 0 or 2 * drop < n


# ---- 7. many recordings ------------------------------------------------------

def test_many_recordings(A, torch, O):
    """Twelve recordings of case C, each at its own tau and length, laid out by
    segments_layout as one batch: each one's phase, sync word and symbols equal
    its own single-stream reference."""
    name = "C"
    freqs, n, hop = R.CASES[name][:3]
    Rn = n // hop
    taus = [64, 128, 192, 16, 80, 144, 208, 10, 75, 140, 250, 3]
    streams = []
    for i, tau in enumerate(taus):
        x, truth = R.case_stream(O, name, tau)
        streams.append((x[:len(x) - 37 * i], truth))
    word = streams[0][1][5:29]
    cfg = A.make_cfg(n=n, hop=hop, freqs=freqs)
    first, count, Wb = A.segments_layout(cfg, [len(x) for x, _ in streams])
    batch = np.zeros((Wb - 1) * hop + n, np.int16)
    for (x, _), f in zip(streams, first):
        batch[int(f) * hop:int(f) * hop + len(x)] = x
    with A.Demodulator(cfg) as d:
        out, res = d.acquire_segments(batch, first, count, sync=word)
    phases = set()
    for s, (x, truth) in enumerate(streams):
        sym, P = O.goertzel(x, freqs, n, hop)
        assert len(sym) == count[s]
        ref_out, ref = R.acquire(sym, P, Rn, word, 0)
        assert R.margin(ref["metric"]) > 4e-5
        for f in INT_FIELDS:
            assert res[s][f] == ref[f], (s, f)
        Mr = ref["metric"]
        assert (np.abs(res[s]["metric"] - Mr) <= MAG_TOL * Mr + ref["per_phase"] * EPS * Mr).all()
        nw = res[s]["n_written"]
        assert nw == ref["n_out"] > 0 and np.array_equal(out[s, :nw], ref_out)
        assert ref["sync_window"] >= 0 and np.array_equal(ref_out, truth[29:29 + nw])
        phases.add(ref["phase"])
    assert phases == set(range(Rn))


# ---- 8. capture and replay ---------------------------------------------------

def test_capture_and_replay(A, torch):
    """demod_batch_async + demod_acquire_segments_async in one graph on a side
    stream: replayed on new PCM, and again after d_first / d_count were
    rewritten in place with another segmentation."""
    name = "A"
    freqs, n, hop = R.CASES[name][:3]
    Rn = n // hop
    from oracle import oracle as O
    refs = []
    for tau in (256, 576):
        x, truth = R.case_stream(O, name, tau)
        refs.append((x, truth) + tuple(O.goertzel(x, freqs, n, hop)))
    W = min(len(r[2]) for r in refs)
    need = (W - 1) * hop + n
    word = refs[0][1][5:29]
    S = 3
    segmentations = [([0, W // 2, 0], [W // 2, W - W // 2, 0]),
                     ([W - 400, 7, 300], [400, 290, W - 700])]
    cap = W // Rn + 1
    with A.Demodulator(n=n, hop=hop, freqs=freqs) as d:
        d_pcm = torch.zeros(need, dtype=torch.int16, device="cuda")
        d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
        d_mag = torch.empty(W * d.k, dtype=torch.float32, device="cuda")
        d_out = torch.empty(S * cap, dtype=torch.uint8, device="cuda")
        d_res = torch.empty(S * RES_BYTES, dtype=torch.uint8, device="cuda")
        d_work = torch.empty(A.acquire_segments_workspace_size(d.cfg, S, W), dtype=torch.uint8,
                             device="cuda")
        d_first, d_count = tables(torch, *segmentations[0])

        def step(stream):
            d.batch_async(d_pcm, W, d_sym, d_mag, stream=stream)
            d.acquire_segments_async(d_sym, d_mag, W, d_first, d_count, S, word, 0, d_out, d_res,
                                     d_work, stream=stream)

        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            d_pcm.copy_(torch.from_numpy(refs[0][0][:need]))     # an eager call of the shape first
            step(side.cuda_stream)
            side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step(torch.cuda.current_stream().cuda_stream)
        found = 0
        for first, count in segmentations:
            nf, nc = tables(torch, first, count)
            d_first.copy_(nf)                                    # in place: the graph holds the pointers
            d_count.copy_(nc)
            for x, truth, sym, P in refs:
                d_pcm.copy_(torch.from_numpy(x[:need]))
                d_res.fill_(0xFF)
                d_out.fill_(0xFF)
                d_work.fill_(0xFF)
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                raw = d_res.cpu().numpy().tobytes()
                out = d_out.cpu().numpy().reshape(S, cap)
                want = SR.acquire_segments(sym[:W], P[:W], Rn, first, count, word, 0)
                for s, (ref_out, ref) in enumerate(want):
                    res = parse(A, raw[s * RES_BYTES:(s + 1) * RES_BYTES])
                    for f in INT_FIELDS:
                        assert res[f] == ref[f], (s, f)
                    Mr = ref["metric"]
                    assert (np.abs(res["metric"] - Mr) <= MAG_TOL * Mr + ref["per_phase"] * EPS * Mr).all()
                    nw = res["n_written"]
                    assert nw == ref["n_out"] and np.array_equal(out[s, :nw], ref_out)
                    assert (out[s, nw:] == 0xFF).all()
                    found += ref["sync_window"] >= 0
        assert found >= 4


# ---- 9. long segments: the finaliser's workgroup path ----------------------------

@pytest.mark.parametrize("Rn,K", [(4, 2), (64, 16), (1, 1)])
def test_long_segments(A, torch, handle, Rn, K):
    """Segments of more than 64 tiles are added, and their phase and first match
    picked, by the finaliser's whole workgroup. One segment X of 66 T + 5
    windows, its word in tile 65, and a second long one Y overlapping it, both
    in one workgroup's four slots (its loop over long segments runs twice), in
    two layouts: the reference's fields, metric and bytes, demod_acquire_async's
    integer fields on the slices, and X's bytes the same in both places."""
    T, L = A.ACQUIRE_TILE, 8
    c0 = 66 * T + 5
    rng = np.random.default_rng(7 + Rn)
    seg_sym, seg_P = make_inputs(c0, K, Rn, 50 + Rn, boost=Rn // 2, flat=True)
    ph = int(np.argmax(R.phase_metric(seg_sym, seg_P, Rn)[0]))
    word = np.zeros(L, np.uint8)
    w0 = ph + ((65 * T) // Rn + 2) * Rn
    if K > 1:
        # the phase's stream is one symbol v everywhere but for the word, which holds
        # six others: no start before the plant comes within one error of it
        a = int(rng.integers(0, K))
        v = (a + 1) % K
        word = np.array([a, a, a, v, a, v, a, a], np.uint8)
        seg_sym[ph::Rn] = v
        seg_sym[w0:w0 + L * Rn:Rn] = word
    ref_out, ref = R.acquire(seg_sym, seg_P, Rn, word, 1)
    assert ref["phase"] == ph and ref["per_phase"] == c0 // Rn
    assert K == 1 or (ref["sync_window"] == w0 and w0 // T == 65)
    cap = c0 // Rn + 1
    d = handle(Rn, K)
    seen = []
    # (slot of X, slot of Y, windows before X): Y = 66 T windows from 700 before X
    for S, sx, sy, lead in ((4, 1, 3, 1500), (6, 0, 2, 707)):
        Wb = lead + c0 + 900
        sym, P = make_inputs(Wb, K, Rn, 60 + S, flat=True)
        sym[lead:lead + c0], P[lead:lead + c0] = seg_sym, seg_P
        first = [int(v) for v in rng.integers(0, Wb - 50, S)]
        count = [int(v) for v in rng.integers(0, 50, S)]
        first[sx], count[sx] = lead, c0
        first[sy], count[sy] = lead - 700, 66 * T
        want = SR.acquire_segments(sym, P, Rn, first, count, word, 1)
        assert want[sy][1]["per_phase"] == 66 * T // Rn
        run = Runner(A, torch, d, sym, P)
        got = run.run(first, count, word, 1, cap, work_windows=3 * Wb)   # overlapping: a wider budget
        check_all(got, want, cap)
        check(got[1][sx], got[0][sx], ref_out, ref, cap)
        whole_batch_agrees(A, torch, d, run, first, count, word, 1, got[1])
        seen.append((got[2][sx], got[0][sx].tobytes()))
    assert seen[0] == seen[1]


# ---- 10. the most segments ------------------------------------------------------

def test_max_segments(A, torch, handle):
    """DEMOD_MAX_SEGMENTS segments of 0, 1 or 2 windows at R = 1, with a
    one-symbol word: 64 rounds of the plan, more tiles than the scan's grid has
    waves (its loop runs again, restaging the LDS), one gather wave a segment.
    At R = 1 with at most two windows everything has a closed form (a sum of
    two doubles has one order): checked for every segment, and the closed form
    against the reference on a sample of them."""
    Rn, K, cap = 1, 2, 2
    S = A.DEMOD_MAX_SEGMENTS
    assert R.RESULT_DTYPE.itemsize == RES_BYTES
    rng = np.random.default_rng(65536)
    count = rng.integers(0, 3, S)
    first = np.cumsum(count + rng.integers(0, 2, S)) - count
    Wb = int(first[-1] + count[-1]) + 3
    assert Wb <= 100000 and int((count > 0).sum()) > 4 * 2048        # tiles > the grid's waves
    sym, P = make_inputs(Wb, K, Rn, 11)
    word = np.array([1], np.uint8)
    d = handle(Rn, K)
    d_sym, d_P = torch.from_numpy(sym).cuda(), torch.from_numpy(P).cuda()
    d_first, d_count = tables(torch, first, count)
    g_out, chk_out = G.guarded(torch, S * cap, torch.uint8, LEAD + 1, LEAD, 0xFF)
    g_res, chk_res = G.guarded(torch, S * RES_BYTES, torch.uint8, LEAD, LEAD, 0xFF)
    g_work, chk_work = G.guarded(torch, A.acquire_segments_workspace_size(d.cfg, S, Wb), torch.uint8,
                                 LEAD, LEAD, 0xFF)
    d.acquire_segments_async(d_sym, d_P, Wb, d_first, d_count, S, word, 0, g_out, g_res, g_work)
    chk_out(written=False)
    chk_res(written=False)
    chk_work(written=False)
    res = np.frombuffer(g_res.cpu().numpy().tobytes(), R.RESULT_DTYPE)
    out = g_out.cpu().numpy().reshape(S, cap)
    # the closed form
    pw = P[np.arange(Wb), sym].astype(np.float64)
    w0, w1 = first, np.minimum(first + 1, Wb - 1)
    M = np.where(count > 0, pw[w0], 0.0) + np.where(count > 1, pw[w1], 0.0)
    hit0 = (count > 0) & (sym[w0] == 1)
    hit1 = (count > 1) & ~hit0 & (sym[w1] == 1)
    sw = np.where(hit0, 0, np.where(hit1, 1, -1))
    fw = np.where(sw >= 0, sw + 1, count)
    n_out = count - fw
    assert np.array_equal(res["metric"][:, 0], M) and not res["metric"][:, 1:].any()
    assert (res["phases"] == 1).all() and not res["phase"].any() and not res["reserved"].any()
    assert np.array_equal(res["per_phase"], count) and np.array_equal(res["sync_window"], sw)
    assert not res["sync_errors"].any() and np.array_equal(res["first_window"], fw)
    assert np.array_equal(res["n_out"], n_out) and np.array_equal(res["n_written"], n_out)
    one = n_out == 1                                    # (a match at window 0 of two: one symbol follows)
    assert np.array_equal(out[one, 0], sym[w1[one]]) and (out[one, 1] == 0xFF).all()
    assert (out[~one] == 0xFF).all() and one.sum() > 1000
    # and the closed form is the reference's, on a sample
    pick = np.r_[0:S:211, S - 50:S]
    want = SR.acquire_segments(sym, P, Rn, first[pick], count[pick], word, 0, cap)
    for s, (ref_out, ref) in zip(pick, want):
        for f in INT_FIELDS + ("n_written",):
            assert res[f][s] == ref[f], (s, f)
        assert res["metric"][s, 0] == ref["metric"][0]
        assert np.array_equal(out[s, :ref["n_written"]], ref_out)
