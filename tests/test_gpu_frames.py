"""The frame scan on the GPU (acquire_frames.hip) against tests/frames_ref.py.

Kernel level: test-made sym / P on the device. Everything is compared by
equality: the powers are small integers, so every order of summing them is
exact and the metric's bytes are the reference's too; where the powers are
arbitrary floats the metric is compared with demod_acquire_async's, byte for
byte, as include/demod.h promises.

End to end: the five-frame stream of tests/frames_ref.py through the sliding
plain bank, the fold-slide and the FFT detector, and a captured graph of batch +
frame scan replayed on two contents with different hit counts.
"""
import ctypes
import functools

import numpy as np
import pytest

import frames_ref as F
import guards as G
from gpu_support import (LEAD, check_frames as check, guarded, handle_fixture, parse_frames as parse, phased,
                         tones_375, torch)  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPE_OF_R = {1: (1024, 1024), 4: (1024, 256), 64: (512, 8)}    # (n, hop) of a handle with R phases
RS, KS = (1, 4, 64), (1, 2, 16)
LS, NS = (1, 24, 64), (0, 1, 7, 64, 300)
MAX_ERRORS = {1: 0, 24: 2, 64: 5}
RES_BYTES = F.RESULT_DTYPE.itemsize
PREFIX = F.RESULT_DTYPE.fields["n_hits"][1]     # metric[64], phases, phase, per_phase: as demod_acquire_result_t
HIT = 16


# handle(R, K): one Demodulator per (R, K), closed with the module.
handle = handle_fixture(lambda A, Rn, K: phased(A, SHAPE_OF_R, Rn, tones_375(K)))


def windows_for(Rn, T):
    return sorted({Rn, T, T + 1, 4 * T + 5, 70001})


def make_inputs(W, K, Rn, seed, target):
    """Background symbols and powers. K >= 2: random symbols < K with a few
    bytes >= K among them; K = 1: 0 and 0xFF half and half (the one symbol and a
    byte that matches nothing). P: the same small integer for every tone of a
    window (sums exact in any order; symbols < K do not move the metric), eight
    times as large on phase `target`."""
    rng = np.random.default_rng(seed)
    if K == 1:
        sym = np.where(rng.integers(0, 2, W) == 1, 0xFF, 0).astype(np.uint8)
    else:
        sym = rng.integers(0, K, W).astype(np.uint8)
        bad = rng.choice(W, W // 40, replace=False)
        sym[bad] = np.array([0x80, 0xFF, K], np.uint8)[np.arange(bad.size) % 3]
    P = np.repeat(rng.integers(1, 1024, (W, 1)).astype(np.float32), K, axis=1)
    P[target::Rn] *= np.float32(8.0)
    return sym, np.ascontiguousarray(P)


def mismatch(v, K, i):
    """A byte that is not symbol v: another symbol < K, or a byte >= K."""
    other = [0x80, 0xFF, K] if K == 1 else [(int(v) + 1) % K, 0x80, (int(v) + K - 1) % K, 0xFF, K]
    return other[i % len(other)]


def plant(sym, Rn, K, w0, word, n_bad, salt=0, keep=()):
    """word on sym[w0 :: Rn] with exactly n_bad mismatching positions (none of
    them in `keep`)."""
    L = len(word)
    sym[w0:w0 + L * Rn:Rn] = word
    free = [i for i in range(L) if i not in keep]
    assert n_bad <= len(free)
    stride = max(1, len(free) // max(n_bad, 1))
    for c, pos in enumerate(free[salt % min(3, stride)::stride][:n_bad]):
        sym[w0 + pos * Rn] = mismatch(word[pos], K, c + salt)
    assert int(np.count_nonzero(sym[w0:w0 + L * Rn:Rn] != word)) == n_bad


class Runner:
    """Device buffers of one (handle, W). run() returns the raw result, its
    dict and the three output arrays whole, rows past n_written included."""

    def __init__(self, A, torch, d, sym, P):
        self.A, self.torch, self.d = A, torch, d
        self.W, self.K = len(sym), P.shape[1]
        self.bits = F.bits_per_symbol(self.K)
        self.d_sym = torch.from_numpy(np.ascontiguousarray(sym)).cuda()
        self.d_P = torch.from_numpy(P).cuda()
        # poisoned once, then whatever the call before left in it
        self.d_work = torch.full((A.frames_workspace_size(d.cfg, self.W),), 0xFF, dtype=torch.uint8,
                                 device="cuda")
        self.d_res = torch.empty(RES_BYTES, dtype=torch.uint8, device="cuda")

    def run(self, word, me, N, max_frames, payload=True, packed=True, stream=0, sym=None, poison=0xFF):
        torch = self.torch
        if sym is not None:
            self.d_sym.copy_(torch.from_numpy(sym))
        B = (N * self.bits + 7) // 8

        def buf(nbytes, want=True):
            return (torch.full((nbytes,), poison, dtype=torch.uint8, device="cuda")
                    if want and nbytes else None)
        d_hits, d_pay, d_pak = buf(max_frames * HIT), buf(max_frames * N, payload), buf(max_frames * B, packed)
        self.d_res.fill_(poison)
        self.d.frames_async(self.d_sym, self.d_P, self.W, word, me, N, d_hits, d_pay, d_pak, max_frames,
                            self.d_res, self.d_work, stream=stream)
        torch.cuda.synchronize()
        raw = self.d_res.cpu().numpy().tobytes()

        def host(t, shape):
            return t.cpu().numpy().reshape(shape) if t is not None else None
        hits = d_hits.cpu().numpy().view(F.HIT_DTYPE) if d_hits is not None else np.zeros(0, F.HIT_DTYPE)
        return dict(raw=raw, res=parse(self.A, raw), hits=hits, payload=host(d_pay, (max_frames, N)),
                    packed=host(d_pak, (max_frames, B)))


def host_rows(t, rows, width):
    return t.cpu().numpy().reshape(rows, width) if t is not None else np.zeros((rows, width), np.uint8)


def plants_for(sym, Rn, K, T, phase, word, me, N):
    """Plants the word on `phase` (see test_plants) into sym wherever the places
    fit the batch and keep clear of each other. Returns (present: {w: errors} of
    the complete ones, absent: [w], tail: the lowest incomplete one or None)."""
    W, L = len(sym), len(word)
    span = (L - 1) * Rn + 1
    taken = []

    def free(w, ph=phase):
        if w < 0 or w % Rn != ph or w + span > W:
            return False
        if any(ph == p2 and abs(w - w2) < span + Rn for w2, p2 in taken):
            return False
        taken.append((w, ph))
        return True

    present, absent, tail = {}, [], None
    # the end of the batch first: the last complete start and, where N >= L
    # leaves room for a second word behind it, the first incomplete one
    c = W - 1 - (L + N - 1) * Rn
    c -= (c - phase) % Rn
    if free(c):
        plant(sym, Rn, K, c, word, me)
        present[c] = me
        if N >= L and free(c + L * Rn):
            plant(sym, Rn, K, c + L * Rn, word, me, salt=1)
            tail = c + L * Rn
    step = span // T + 2                      # tiles between two plants' edges
    edges = iter(range(T, W, step * T))
    places = [("last", lambda e: e - Rn + phase, me), ("first", lambda e: e + phase, me)]
    if L > 1:
        places += [("split", (lambda s: lambda e: e + phase - s * Rn)(s), me)
                   for s in sorted({2 % L, L // 2, L - 1})]
        places += [("worse", lambda e: e + phase - (L // 2) * Rn, me + 1)]
    places += [("worse", lambda e: e + phase, me + 1)]
    if Rn > 1:
        places += [("other", lambda e: e + (phase + 1) % Rn, 0)]
    for (kind, at, n_bad), e in zip(places, edges):
        w = at(e)
        if n_bad >= L and kind == "worse":    # a one-symbol word has no worse copy but a miss
            n_bad = L
        if kind == "other":
            if free(w, (phase + 1) % Rn):
                plant(sym, Rn, K, w, word, 0)
            continue
        if not free(w):
            continue
        plant(sym, Rn, K, w, word, n_bad, salt=len(taken))
        if n_bad > me:
            absent.append(w)
        elif w + (L + N - 1) * Rn < W:
            present[w] = n_bad
        elif tail is None or w < tail:         # a hit whose frame leaves the batch
            tail = w
    return present, absent, tail


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("Rn", RS)
def test_plants(A, torch, handle, Rn, K):
    """Every (W, L, N) at this (R, K), one run each: the word planted with
    exactly max_errors mismatches at the last start of a tile on the phase, the
    first start of a tile, starts whose word straddles a tile edge at three
    splits, the last complete start and (N >= L) a first incomplete start
    behind it; copies with one more mismatch and a clean copy on the next
    phase. The planted hits are in the list with their error counts, the worse
    and other-phase copies are not, and result, hits, payload and packed bytes
    equal the reference's."""
    T = A.ACQUIRE_TILE
    d = handle(Rn, K)
    full = 0
    for W in windows_for(Rn, T):
        target = (W * 7 + K) % Rn
        base, P = make_inputs(W, K, Rn, 1000 * Rn + 10 * K + W % 7, target)
        run = Runner(A, torch, d, base, P)
        for L in LS:
            me = MAX_ERRORS[L]
            rng = np.random.default_rng(L + W)
            word = rng.integers(0, K, L).astype(np.uint8)
            for N in NS:
                sym = base.copy()
                present, absent, tail = plants_for(sym, Rn, K, T, target, word, me, N)
                ref = F.frames(sym, P, Rn, word, me, N)
                r_res = ref[3]
                if W >= T:
                    assert r_res["phase"] == target          # the fixture's condition
                cap = r_res["n_hits"] + 3
                out = run.run(word, me, N, cap, sym=sym)
                check(A, out, ref, cap)
                if r_res["phase"] != target:
                    continue
                got = dict(zip(out["hits"]["window"][:r_res["n_hits"]].tolist(),
                               out["hits"]["errors"][:r_res["n_hits"]].tolist()))
                for w, e in present.items():
                    assert got.get(w) == e, (W, L, N, w, e, got.get(w))
                for w in absent:
                    assert w not in got, (W, L, N, w)
                assert all(w % Rn == target for w in got)
                if tail is not None:        # (the background may hold an incomplete hit before it)
                    assert 0 <= out["res"]["tail_window"] <= tail
                    assert out["res"]["tail_window"] < tail or out["res"]["tail_errors"] == me
                if N == 0:
                    assert out["res"]["tail_window"] == -1
                full += W == 70001 and len(present) >= (5 if L > 1 else 3) and len(absent) >= 1
    assert full == len(LS) * len(NS)       # at 70 001 windows every place was planted


@pytest.mark.parametrize("Rn,K", [(1, 2), (4, 16), (64, 2), (4, 1)])
def test_overlapping_hits(A, torch, handle, Rn, K):
    """Two hits one symbol (R windows) apart: at a tile edge, and as the last
    complete start with the first incomplete one right behind it (the tail).
    The word is two runs, so a copy shifted by one symbol is one error away."""
    T = A.ACQUIRE_TILE
    W = 4 * T + 5
    d = handle(Rn, K)
    target = Rn // 2
    base, P = make_inputs(W, K, Rn, 5 + Rn + K, target)
    run = Runner(A, torch, d, base, P)
    c0, c1 = (0, 0) if K == 1 else (1, 0)
    for L, me in ((1, 0), (24, 2), (64, 5)):
        if L * Rn * 2 > W:
            continue
        h = L // 2
        word = np.array([c0] * h + [c1] * (L - h), np.uint8)
        for N in (1, 7, 64):
            sym = base.copy()
            c = W - 1 - (L + N - 1) * Rn
            c -= (c - target) % Rn
            if c < 0:                          # no complete frame fits this batch
                continue
            pairs = [c]
            a = 2 * T - Rn + target            # the last start of tile 1; a + R is tile 2's first
            if a + (L + 1) * Rn + Rn < c:
                pairs.append(a)
            for w in pairs:
                # L + 1 symbols, the second run one longer: errors(w) = 0, errors(w + R) = [c0 != c1]
                seq = np.concatenate([word[:h + 1] if L > 1 else word, word[h:] if L > 1 else word])
                sym[w:w + len(seq) * Rn:Rn] = seq
            ref = F.frames(sym, P, Rn, word, me, N)
            assert ref[3]["phase"] == target
            cap = ref[3]["n_hits"] + 1
            out = run.run(word, me, N, cap, sym=sym)
            check(A, out, ref, cap)
            got = out["hits"]["window"][:ref[3]["n_hits"]].tolist()
            assert c in got and out["res"]["tail_window"] == c + Rn
            if len(pairs) > 1:
                assert a in got and a + Rn in got and got.index(a + Rn) == got.index(a) + 1


@pytest.mark.parametrize("Rn", RS)
def test_every_start_hits(A, torch, handle, Rn):
    """K = 1, L = 1, W = 4 T + 5, all symbols 0: every start on the phase is a
    hit. The whole list in order, n_hits exact; max_frames below, at and above
    n_hits, rows past n_written untouched, guards around every output."""
    T = A.ACQUIRE_TILE
    W, K, N = 4 * T + 5, 1, 7
    d = handle(Rn, K)
    target = Rn - 1
    sym = np.zeros(W, np.uint8)
    P = np.ones((W, 1), np.float32)
    P[target::Rn] = 8.0
    word = np.zeros(1, np.uint8)
    ref = F.frames(sym, P, Rn, word, 0, N)
    n_hits = ref[3]["n_hits"]
    starts = np.arange(target, W, Rn)
    assert n_hits == int(np.count_nonzero(starts + N * Rn < W)) and ref[3]["phase"] == target
    assert ref[0]["window"].tolist() == starts[:n_hits].tolist()
    assert ref[3]["tail_window"] == starts[n_hits]
    d_sym, d_P = torch.from_numpy(sym).cuda(), torch.from_numpy(P).cuda()
    work_bytes = A.frames_workspace_size(d.cfg, W)
    for cap in (0, 1, n_hits - 1, n_hits, n_hits + 5):
        g_hits, chk_hits = guarded(torch, cap * HIT, LEAD, 0xFF)
        g_pay, chk_pay = guarded(torch, cap * N, LEAD + 1, 0xFF)
        g_pak, chk_pak = guarded(torch, cap * 1, LEAD + 3, 0xFF)
        g_res, chk_res = guarded(torch, RES_BYTES, LEAD, 0xFF)
        g_work, chk_work = guarded(torch, work_bytes, LEAD, 0xFF)
        d.frames_async(d_sym, d_P, W, word, 0, N, g_hits, g_pay, g_pak, cap, g_res, g_work)
        for chk in (chk_hits, chk_pay, chk_pak, chk_res, chk_work):
            chk(written=False)
        raw = g_res.cpu().numpy().tobytes()
        out = dict(raw=raw, res=parse(A, raw), hits=host_rows(g_hits, cap, HIT).reshape(-1).view(F.HIT_DTYPE),
                   payload=host_rows(g_pay, cap, N), packed=host_rows(g_pak, cap, 1))
        check(A, out, ref, cap)
        assert out["res"]["n_hits"] == n_hits and out["res"]["n_written"] == min(cap, n_hits)


def float_inputs(W, K, Rn, seed, boost):
    """Powers over 14 decades: sums that depend on their order."""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, K, W).astype(np.uint8)
    sym[rng.choice(W, W // 50 + 1, replace=False)] = 0xFF
    P = (10.0 ** rng.uniform(0.0, 14.0, (W, K))).astype(np.float32)
    P[boost::Rn] *= np.float32(1.5)
    return sym, np.ascontiguousarray(P)


@pytest.mark.parametrize("Rn", RS)
def test_phase_decision_is_the_acquisition(A, torch, handle, Rn):
    """metric, phases, phase and per_phase are byte-equal to
    demod_acquire_async's on the same tensors, and hits[0].window is its
    sync_window whenever the lowest hit is complete."""
    T = A.ACQUIRE_TILE
    firsts = 0
    for K in KS:
        d = handle(Rn, K)
        for W in windows_for(Rn, T):
            sym, P = float_inputs(W, K, Rn, 3 * W + K, (W + K) % Rn)
            run = Runner(A, torch, d, sym, P)
            d_awork = torch.empty(A.acquire_workspace_size(d.cfg), dtype=torch.uint8, device="cuda")
            d_ares = torch.empty(ctypes.sizeof(A.DemodAcquireResult), dtype=torch.uint8, device="cuda")
            for L in (1, 3):
                word = np.arange(L, dtype=np.uint8) % K
                for N in (0, 7):
                    out = run.run(word, 0, N, 4)
                    d.acquire_async(run.d_sym, run.d_P, W, word, 0, None, d_ares, d_awork)
                    torch.cuda.synchronize()
                    araw = d_ares.cpu().numpy().tobytes()
                    assert out["raw"][:PREFIX] == araw[:PREFIX]
                    acq = A.acquire_result_dict(A.DemodAcquireResult.from_buffer_copy(araw))
                    ref = F.frames(sym, P, Rn, word, 0, N, max_frames=4)
                    res = out["res"]
                    # equal phases: the rest is integers and must be the reference's
                    if ref[3]["phase"] == res["phase"]:
                        for f in ("n_hits", "n_written", "tail_window", "tail_errors"):
                            assert res[f] == ref[3][f], f
                        assert out["hits"][:res["n_written"]].tobytes() == ref[0].tobytes()
                    # the acquisition stops at the lowest hit, complete or not
                    first = int(out["hits"]["window"][0]) if res["n_hits"] else -1
                    tail = res["tail_window"]
                    if first >= 0 and (tail < 0 or first < tail):
                        assert acq["sync_window"] == first
                        assert acq["sync_errors"] == int(out["hits"]["errors"][0])
                        firsts += 1
                    else:
                        assert acq["sync_window"] == tail and acq["sync_errors"] == res["tail_errors"]
    assert firsts >= 10


def test_determinism_and_second_stream(A, torch, handle):
    """Two runs, and a run on a second stream with buffers of its own, give
    byte-identical outputs."""
    Rn, K, W, N = 4, 2, 70001, 64
    sym, P = float_inputs(W, K, Rn, 11, 1)
    word = np.array([1, 0, 1], np.uint8)
    d = handle(Rn, K)
    run = Runner(A, torch, d, sym, P)
    ref = F.frames(sym, P, Rn, word, 1, N)
    cap = ref[3]["n_hits"] + 2
    assert ref[3]["n_hits"] > 1000
    o1 = run.run(word, 1, N, cap)
    o2 = run.run(word, 1, N, cap)
    side = torch.cuda.Stream()
    other = Runner(A, torch, d, sym, P)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        o3 = other.run(word, 1, N, cap, stream=side.cuda_stream)
    for o in (o2, o3):
        assert o["raw"] == o1["raw"]
        for f in ("hits", "payload", "packed"):
            assert o[f].tobytes() == o1[f].tobytes(), f
    if o1["res"]["phase"] == ref[3]["phase"]:
        assert o1["hits"][:ref[3]["n_hits"]].tobytes() == ref[0].tobytes()
        assert np.array_equal(o1["payload"][:ref[3]["n_hits"]], ref[1])
        assert np.array_equal(o1["packed"][:ref[3]["n_hits"]], ref[2])


@pytest.mark.parametrize("Rn,K,W,L,N", [(4, 2, 4101, 3, 7), (64, 2, 1025, 1, 1), (1, 16, 5000, 2, 300),
                                        (1, 2, 1, 1, 0), (4, 1, 70001, 24, 64)])
def test_guards(A, torch, handle, Rn, K, W, L, N):
    """d_hits, d_payload, d_packed (odd alignments), d_result and d_work between
    poisoned guards; max_frames below and above n_hits; d_work poisoned with
    0xFF, with 0x5A, and holding the previous call's contents: the same bytes
    every time, every byte of d_result written, sym and P unchanged."""
    d = handle(Rn, K)
    target = (W + K) % Rn
    sym, P = make_inputs(W, K, Rn, 21 + W, target)
    word = (np.arange(L) % K).astype(np.uint8) if L < 24 else np.zeros(L, np.uint8)
    me = 0 if L < 24 else 12
    bits = F.bits_per_symbol(K)
    B = (N * bits + 7) // 8
    ref = F.frames(sym, P, Rn, word, me, N)
    n_hits = ref[3]["n_hits"]
    g_sym, chk_sym = G.guarded(torch, W, torch.uint8, LEAD + 3, LEAD, 0xFF)
    g_sym.copy_(torch.from_numpy(sym))
    g_P, chk_P = G.guarded(torch, W * K, torch.float32, G.F32_GUARD + 1, G.F32_GUARD, G.F32_POISON)
    g_P.copy_(torch.from_numpy(P.reshape(-1)))
    work_bytes = A.frames_workspace_size(d.cfg, W)
    assert n_hits > 0 or W == 1              # the fixture's condition
    for cap in sorted({max(n_hits - 1, 0), n_hits + 7, 1}):
        raws = []
        g_work, chk_work = guarded(torch, work_bytes, LEAD, 0xFF)
        for poison in (0xFF, 0x5A, None):       # None: d_work as the call before left it
            if poison is not None:
                g_work.fill_(poison)
            out_poison = poison or 0xFF
            g_hits, chk_hits = guarded(torch, cap * HIT, LEAD, out_poison)
            g_pay, chk_pay = guarded(torch, cap * N, LEAD + 1, out_poison)
            g_pak, chk_pak = guarded(torch, cap * B, LEAD + 3, out_poison)
            g_res, chk_res = guarded(torch, RES_BYTES, LEAD, out_poison)
            d.frames_async(g_sym, g_P, W, word, me, N, g_hits, g_pay, g_pak, cap, g_res, g_work)
            for chk in (chk_hits, chk_pay, chk_pak, chk_res, chk_work):
                chk(written=False)
            raw = g_res.cpu().numpy().tobytes()
            out = dict(raw=raw, res=parse(A, raw),
                       hits=host_rows(g_hits, cap, HIT).reshape(-1).view(F.HIT_DTYPE),
                       payload=host_rows(g_pay, cap, N), packed=host_rows(g_pak, cap, B))
            check(A, out, ref, cap, out_poison)
            raws.append(raw)
        assert raws[0] == raws[1] == raws[2]     # no byte of d_result was left unwritten
    chk_sym(written=False)
    chk_P(written=False)
    assert np.array_equal(g_sym.cpu().numpy(), sym)
    assert np.array_equal(g_P.cpu().numpy().view(np.int32), P.reshape(-1).view(np.int32))


def test_refusals(A, torch, handle):
    """Every DEMOD_BAD_ARG case returns without a launch: the outputs stay poison."""
    lib = A.load_library()
    K, W, N, cap = 8, 4096, 16, 64
    d = A.Demodulator(n=1024, hop=256, freqs=tuple(1500.0 + 375.0 * i for i in range(K)))
    sym, P = make_inputs(W, K, 4, 1, 0)
    d_sym, d_P = torch.from_numpy(sym).cuda(), torch.from_numpy(P).cuda()

    def poison(nbytes):
        return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    work_bytes = A.frames_workspace_size(d.cfg, W)
    d_hits, d_pay, d_pak = poison(cap * HIT), poison(cap * N), poison(cap * N)
    d_res, d_work = poison(RES_BYTES + 8), poison(work_bytes + 8)
    good = np.arange(8, dtype=np.uint8)
    ps, pm, ph, pp, pk, pr, pw = (t.data_ptr() for t in (d_sym, d_P, d_hits, d_pay, d_pak, d_res, d_work))
    sp = good.ctypes.data
    bad_sym = np.array([0, K], np.uint8)
    long_word = np.zeros(65, np.uint8)

    def call(h=d._h, sym_p=ps, mag_p=pm, n_windows=W, sync=sp, sync_len=8, max_errors=0, n=N, hits_p=ph,
             pay_p=pp, pak_p=pk, max_frames=cap, res_p=pr, work_p=pw, wb=work_bytes):
        return lib.demod_frames_async(h, sym_p, mag_p, n_windows, sync, sync_len, max_errors, n, hits_p,
                                      pay_p, pak_p, max_frames, res_p, work_p, wb, None)

    cases = dict([
        ("W < R", dict(n_windows=3)),
        ("W >= 2^31", dict(n_windows=2 ** 31)),
        ("sync_len > 64", dict(sync=long_word.ctypes.data, sync_len=65)),
        ("sync symbol >= K", dict(sync=bad_sym.ctypes.data, sync_len=2)),
        ("max_errors >= sync_len", dict(max_errors=8)),
        ("NULL sync", dict(sync=None)),
        ("sync_len == 0", dict(sync_len=0)),
        ("sync_len == 0, NULL sync", dict(sync=None, sync_len=0)),
        ("(L + N) R >= 2^31", dict(n=2 ** 29 - 8)),
        ("NULL d_symbols", dict(sym_p=None)),
        ("NULL d_mags", dict(mag_p=None)),
        ("NULL d_result", dict(res_p=None)),
        ("NULL d_work", dict(work_p=None)),
        ("NULL d_hits with max_frames", dict(hits_p=None)),
        ("max_frames >= 2^31", dict(max_frames=2 ** 31)),
        ("work_bytes short", dict(wb=work_bytes - 1)),
        ("misaligned d_hits", dict(hits_p=ph + 4)),
        ("misaligned d_result", dict(res_p=pr + 4)),
        ("misaligned d_work", dict(work_p=pw + 4, wb=work_bytes + 4)),
        ("NULL handle", dict(h=None)),
    ])
    others = [A.Demodulator(n=1024, hop=384, freqs=(1500.0, 3000.0)),
              A.Demodulator(n=1024, hop=8, freqs=(1500.0, 3000.0))]
    try:
        for what, kw in cases.items():
            assert call(**kw) == A.DEMOD_BAD_ARG, what
        for dd, what in zip(others, ("n % hop != 0", "R > 64")):
            assert call(h=dd._h, sync_len=1) == A.DEMOD_BAD_ARG, what
            with pytest.raises(A.DemodError) as e:
                dd.frames(np.zeros(4096, np.int16), good[:2])
            assert e.value.code == A.DEMOD_BAD_ARG
        # the Python mirror's own checks (before any pointer reaches the library)
        full = dict(d_sym=d_sym, d_mag=d_P.reshape(-1), d_hits=d_hits, d_payload=d_pay, d_packed=d_pak,
                    d_result=d_res, d_work=d_work)
        for kw in (dict(d_sym=d_sym[:W - 1]), dict(d_mag=d_P.reshape(-1)[:W * K - 1]),
                   dict(d_hits=d_hits[:cap * HIT - 1]), dict(d_hits=None), dict(d_payload=d_pay[:cap * N - 1]),
                   dict(d_packed=d_pak[:cap * N * 3 // 8 - 1]), dict(d_result=d_res[:RES_BYTES - 1]),
                   dict(d_work=d_work[:work_bytes - 1]), dict(d_sym=d_sym.cpu()),
                   dict(d_result=d_res.to(torch.int16))):
            a = dict(full)
            a.update(kw)
            with pytest.raises(A.DemodError) as e:
                d.frames_async(a["d_sym"], a["d_mag"], W, good, 0, N, a["d_hits"], a["d_payload"],
                               a["d_packed"], cap, a["d_result"], a["d_work"])
            assert e.value.code == A.DEMOD_BAD_ARG
        torch.cuda.synchronize()
        for t in (d_hits, d_pay, d_pak, d_res, d_work):
            assert bool((t == 0xFF).all()), "a refused call wrote"
        # and the same call, legal, runs; so does a count-only one
        d.frames_async(d_sym, d_P.reshape(-1), W, good, 0, N, d_hits, d_pay, d_pak, cap, d_res, d_work)
        torch.cuda.synchronize()
        first = parse(A, d_res[:RES_BYTES].cpu().numpy().tobytes())
        assert first["phases"] == 4
        d_res.fill_(0xFF)
        d.frames_async(d_sym, d_P.reshape(-1), W, good, 0, N, None, None, None, 0, d_res, d_work)
        torch.cuda.synchronize()
        count = parse(A, d_res[:RES_BYTES].cpu().numpy().tobytes())
        assert count["n_written"] == 0 and count["n_hits"] == first["n_hits"]
        # the longest legal frame, (L + N) R = 2^31 - 4: nothing is complete
        assert call(n=2 ** 29 - 9, max_frames=0, hits_p=None) == A.DEMOD_OK
        torch.cuda.synchronize()
        assert parse(A, d_res[:RES_BYTES].cpu().numpy().tobytes())["n_hits"] == 0
    finally:
        for dd in others + [d]:
            dd.close()


# ---- end to end --------------------------------------------------------------

DETECTORS = {"slide": (F.FSK2, "METHOD_AUTO"), "fold_slide": (F.FSK8, "METHOD_AUTO"),
             "fft": (F.FSK2, "METHOD_FFT")}


@functools.lru_cache(maxsize=None)
def stream_reference(freqs, tau, drop=()):
    """(x, word, payloads, windows, reference on the oracle's double powers):
    computed once per plan, tau and drop."""
    from oracle import oracle as O
    x, word, payloads, windows = F.frame_stream(freqs, tau, drop=drop)
    sym, P = O.goertzel(x, freqs, 1024, 256)
    return x, word, payloads, windows, F.frames(sym, P, 4, word, 1, F.FRAME_N)


@pytest.mark.parametrize("name", sorted(DETECTORS))
def test_end_to_end(A, torch, name):
    """The five-frame stream at three tau through one sliding detector, via
    Demodulator.frames on a host array and on a device tensor: windows,
    payloads and packed bytes equal the planted truth and the reference."""
    freqs, method = DETECTORS[name]
    bits = F.bits_per_symbol(len(freqs))
    with A.Demodulator(n=1024, hop=256, freqs=freqs, method=getattr(A, method)) as d:
        assert d.method == {"slide": A.METHOD_GOERTZEL, "fold_slide": A.METHOD_FOLDED,
                            "fft": A.METHOD_FFT}[name]
        assert name == "fft" or d.slide_windows > 0
        for tau in F.FRAME_TAUS:
            x, word, payloads, windows, ref = stream_reference(freqs, tau)
            r_hits, r_pay, r_pak, r_res = ref
            # the fixture's condition, on the reference alone
            assert r_hits["window"].tolist() == windows.tolist() and np.array_equal(r_pay, payloads)
            assert r_res["phase"] == (tau + 128) // 256 and r_res["tail_window"] == -1
            for pcm in (x, torch.from_numpy(x).cuda()):
                hits, pay, pak, res = d.frames(pcm, word, max_errors=1, frame_symbols=F.FRAME_N)
                assert res["phase"] == r_res["phase"] and res["per_phase"] == r_res["per_phase"]
                assert res["n_hits"] == res["n_written"] == F.FRAME_COUNT and res["tail_window"] == -1
                assert hits.tobytes() == r_hits.tobytes()
                assert hits["window"].tolist() == windows.tolist()
                assert np.array_equal(pay, payloads) and np.array_equal(pay, r_pay)
                assert np.array_equal(pak, r_pak) and np.array_equal(pak, F.pack(payloads, bits))
                err = np.abs(res["metric"] - r_res["metric"])
                assert (err <= (G.MAG_TOL + r_res["per_phase"] * 2.0 ** -52) * r_res["metric"]).all()
            # a short max_frames cuts the list, not the count; payload alone
            hits, pay, pak, res = d.frames(x, word, max_errors=1, frame_symbols=F.FRAME_N, max_frames=2,
                                           packed=False)
            assert res["n_hits"] == F.FRAME_COUNT and res["n_written"] == 2 and pak is None
            assert hits.tobytes() == r_hits[:2].tobytes() and np.array_equal(pay, payloads[:2])


def test_capture_and_replay(A, torch):
    """demod_batch_async + demod_frames_async in one graph on a side stream,
    replayed on two contents with different hit counts: each replay's bytes
    are the eager bytes for that content, and the reference's."""
    freqs, N, cap = F.FSK2, F.FRAME_N, 8
    refs = [stream_reference(freqs, 256), stream_reference(freqs, 256, (1, 3))]
    assert [r[4][3]["n_hits"] for r in refs] == [5, 3]
    W = (len(refs[0][0]) - 1024) // 256 + 1
    assert len(refs[1][0]) == len(refs[0][0])
    word = refs[0][1]
    with A.Demodulator(n=1024, hop=256, freqs=freqs) as d:
        d_pcm = torch.zeros(len(refs[0][0]), dtype=torch.int16, device="cuda")
        d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
        d_mag = torch.empty(W * d.k, dtype=torch.float32, device="cuda")
        outs = [torch.empty(nb, dtype=torch.uint8, device="cuda")
                for nb in (cap * HIT, cap * N, cap * N // 8, RES_BYTES)]
        d_work = torch.empty(A.frames_workspace_size(d.cfg, W), dtype=torch.uint8, device="cuda")

        def step(stream):
            d.batch_async(d_pcm, W, d_sym, d_mag, stream=stream)
            d.frames_async(d_sym, d_mag, W, word, 1, N, outs[0], outs[1], outs[2], cap, outs[3], d_work,
                           stream=stream)

        def results():
            torch.cuda.synchronize()
            return [t.cpu().numpy().tobytes() for t in outs]

        side = torch.cuda.Stream()
        eager = []
        with torch.cuda.stream(side):
            for x, *_ in refs:                            # eager calls of the shape first
                d_pcm.copy_(torch.from_numpy(x))
                for t in outs:
                    t.fill_(0xFF)
                step(side.cuda_stream)
                side.synchronize()
                eager.append(results())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step(torch.cuda.current_stream().cuda_stream)
        for rep in range(2):
            for i, (x, *_) in enumerate(refs):
                d_pcm.copy_(torch.from_numpy(x))
                for t in outs:
                    t.fill_(0xFF)
                torch.cuda.synchronize()
                g.replay()
                assert results() == eager[i], (rep, i)
        for got, (x, word_i, payloads, windows, ref) in zip(eager, refs):
            res = parse(A, got[3])
            n = ref[3]["n_hits"]
            assert res["n_hits"] == res["n_written"] == n and res["phase"] == 1
            hits = np.frombuffer(got[0], F.HIT_DTYPE)
            assert hits[:n].tobytes() == ref[0].tobytes()
            assert (np.frombuffer(got[0], np.uint8)[n * HIT:] == 0xFF).all()
            assert np.array_equal(np.frombuffer(got[1], np.uint8).reshape(cap, N)[:n], ref[1])
            assert np.array_equal(np.frombuffer(got[2], np.uint8).reshape(cap, N // 8)[:n], ref[2])
