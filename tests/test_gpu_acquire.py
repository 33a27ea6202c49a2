"""Acquisition on the GPU (acquire.hip) against tests/acquire_ref.py.

Kernel level: test-made sym / P on the device, every phase count R a handle
can have (n and hop are powers of two, so R = n / hop is 1, 2, 4, .. 64; an odd
R cannot be configured and demod_acquire_async refuses it), K in {1, 2, 8, 16},
window counts around R and around the scan's tile T = ACQUIRE_TILE.

  metric   |M - M_ref| <= J 2^-52 M_ref: M_ref is the correctly rounded sum
           (math.fsum), and any order of summing J non-negative doubles is
           within (J - 1) 2^-53 (1 + o(1)) of the exact sum. Derived, not
           measured.
  phase, sync_window, sync_errors, first_window, n_out, n_written and the
  output bytes: equal to the reference's.

End to end: cases A-D of DESIGN.md §4.9 through the detectors, and a captured
graph of batch + acquisition replayed on two contents.
"""
import functools

import numpy as np
import pytest

import acquire_ref as R
import guards as G
from acquire_ref import make_inputs, plant
from guards import MAG_TOL
from gpu_support import (EPS, check_acquire as check, handle_fixture, parse_acquire as parse, phased, tones_375,
                         torch)  # noqa: F401

pytestmark = pytest.mark.gpu

# (n, hop) of a handle with R = n / hop phases
SHAPE_OF_R = {1: (1024, 1024), 2: (1024, 512), 4: (1024, 256), 8: (1024, 128), 16: (1024, 64),
              32: (256, 8), 64: (512, 8)}
RS = sorted(SHAPE_OF_R)
KS = (1, 2, 8, 16)
RES_BYTES = R.RESULT_DTYPE.itemsize
LEAD = 4096          # guard bytes per side (a multiple of 8: d_result and d_work stay aligned)


# handle(R, K): one Demodulator per (R, K), closed with the module.
handle = handle_fixture(lambda A, Rn, K: phased(A, SHAPE_OF_R, Rn, tones_375(K)))


class Runner:
    """Device buffers of one (handle, W): run(sym, sync, max_errors, cap)."""

    def __init__(self, A, torch, d, sym, P):
        self.A, self.torch, self.d = A, torch, d
        self.W = len(sym)
        self.d_sym = torch.from_numpy(np.ascontiguousarray(sym)).cuda()
        self.d_P = torch.from_numpy(P).cuda()
        self.d_work = torch.empty(A.acquire_workspace_size(d.cfg), dtype=torch.uint8, device="cuda")
        self.d_res = torch.empty(RES_BYTES, dtype=torch.uint8, device="cuda")

    def run(self, sync=None, max_errors=0, cap=0, stream=0, sym=None):
        torch = self.torch
        if sym is not None:
            self.d_sym.copy_(torch.from_numpy(sym))
        d_out = torch.full((cap,), 0xFF, dtype=torch.uint8, device="cuda") if cap else None
        self.d_res.fill_(0xFF)
        self.d.acquire_async(self.d_sym, self.d_P, self.W, sync, max_errors, d_out, self.d_res,
                             self.d_work, stream=stream)
        torch.cuda.synchronize()
        raw = self.d_res.cpu().numpy().tobytes()
        res = parse(self.A, raw)
        out = d_out.cpu().numpy() if cap else np.zeros(0, np.uint8)
        return out, res, raw


def windows_for(Rn, T):
    return sorted({w for w in (Rn, Rn + 1, 2 * Rn - 1, T, T + 1, 4 * T + 5, 70001) if w >= Rn})


@pytest.mark.parametrize("Rn", RS)
def test_metric_phase_and_stream(A, torch, handle, Rn):
    """Every (K, W) at this R: metric within the summation bound, phase and
    the sync-less output stream equal to the reference's; then a planted word."""
    T = A.ACQUIRE_TILE
    found = 0
    for K in KS:
        d = handle(Rn, K)
        for W in windows_for(Rn, T):
            boost = (W * 7 + K) % Rn
            sym, P = make_inputs(W, K, Rn, 1000 * Rn + 10 * K + W % 7, boost)
            ref_out, ref = R.acquire(sym, P, Rn)
            assert Rn == 1 or R.margin(ref["metric"]) > 1e-6     # the reference's own margin
            run = Runner(A, torch, d, sym, P)
            cap = W // Rn + 3
            out, res, _ = run.run(cap=cap)
            check(res, out, ref_out, ref, cap)
            assert res["sync_window"] == -1 and res["first_window"] == ref["phase"]
            # a word of 5 planted on the reference's phase, one error allowed
            if W >= 8 * Rn:
                word = ((np.arange(5) * 3 + 1) % K).astype(np.uint8)
                s2 = sym.copy()
                w0 = ref["phase"] + (W // Rn - 6) // 2 * Rn
                s2[w0:w0 + 5 * Rn:Rn] = word
                s2[w0 + 2 * Rn] = 0x80                              # a byte >= K: one error
                ref_out, ref2 = R.acquire(s2, P, Rn, word, 1)
                out, res, _ = run.run(word, 1, cap, sym=s2)
                check(res, out, ref_out, ref2, cap)
                # (the planted symbols pick other powers: the phase may move off the word)
                found += ref2["sync_window"] >= 0
    assert found >= 8


SWEEPS = [
    (1, 2, 1, 0), (1, 8, 24, 3), (1, 16, 64, 5),
    (2, 8, 1, 0), (2, 2, 24, 2), (2, 8, 64, 0),
    (16, 16, 1, 0), (16, 8, 24, 3), (16, 2, 64, 7),
    (64, 2, 1, 0), (64, 16, 24, 0), (64, 8, 64, 5),
]


def sweep_inputs(T, Rn, K, L, max_errors):
    """The sync sweep's background: (sym, P, word, phase, metric). The phase's
    own symbols never match a one-symbol word; longer words over random
    symbols have no match within max_errors (asserted by the caller)."""
    rng = np.random.default_rng(77 * Rn + L)
    W = 2 * T + Rn + L * Rn + 5
    # the powers span 14 decades, so the largest few decide the phase, not
    # the 1.5: the sweep runs on whichever phase the reference finds
    sym, P = make_inputs(W, K, Rn, 5 + Rn + L, boost=(3 * L + 1) % Rn, flat=True)
    phase = int(np.argmax(R.phase_metric(sym, P, Rn)[0]))
    word = rng.integers(0, K, L).astype(np.uint8)
    if L == 1:
        sym[phase::Rn] = (int(word[0]) + 1) % K      # other phases stay random: they hold matches
    return sym, P, word, phase, R.phase_metric(sym, P, Rn), rng


def sweep_plants(T, Rn, K, L, max_errors):
    """(p, n_bad, sym with the word planted at p with n_bad mismatches, reference)."""
    sym, P, word, phase, metric, rng = sweep_inputs(T, Rn, K, L, max_errors)
    assert int(np.argmax(metric[0])) == phase and (Rn == 1 or R.margin(metric[0]) > 1e-6)
    _, ref0 = R.acquire(sym, P, Rn, word, max_errors, metric=metric)
    assert ref0["sync_window"] == -1                     # no match to begin with
    for p in range(phase, 2 * T + Rn, Rn):
        for n_bad in (max_errors, max_errors + 1):
            s = plant(sym, Rn, p, word, n_bad, K, rng)
            ref_out, ref = R.acquire(s, P, Rn, word, max_errors, metric=metric)
            # what the plant must give, by the definitions alone
            if n_bad == max_errors:
                assert ref["sync_window"] == p and ref["sync_errors"] == max_errors
            else:
                assert ref["sync_window"] == -1 and ref["n_out"] == 0
            yield p, n_bad, s, ref_out, ref


@pytest.mark.parametrize("Rn,K,L,max_errors", SWEEPS)
def test_sync_at_every_start(A, torch, handle, Rn, K, L, max_errors):
    """The word planted at every start p in [0, 2 T + R) on the phase, one run
    per p: found with exactly max_errors mismatches (sync_errors exact), not
    found with one more."""
    T = A.ACQUIRE_TILE
    sym, P, word, phase = sweep_inputs(T, Rn, K, L, max_errors)[:4]
    run = Runner(A, torch, handle(Rn, K), sym, P)
    cap = len(sym) // Rn + 1
    runs = 0
    for p, n_bad, s, ref_out, ref in sweep_plants(T, Rn, K, L, max_errors):
        out, res, _ = run.run(word, max_errors, cap, sym=s)
        check(res, out, ref_out, ref, cap, metric=(runs == 0))
        runs += 1
    assert runs == 2 * len(range(phase, 2 * T + Rn, Rn))


@pytest.mark.parametrize("Rn,K,L", [(4, 8, 24), (1, 16, 64), (64, 8, 24), (8, 16, 1)])
def test_sync_rules(A, torch, handle, Rn, K, L):
    """Another phase's earlier perfect match is ignored; of two matches the
    first wins; the last legal start is found and one window later is not; no
    match gives -1 and an empty stream."""
    T = A.ACQUIRE_TILE
    rng = np.random.default_rng(9 * Rn + L)
    W = max(3 * T + 17, (2 * L + 10) * Rn + 3)
    sym, P = make_inputs(W, K, Rn, 31 + Rn, boost=Rn // 2, flat=True)
    phase = int(np.argmax(R.phase_metric(sym, P, Rn)[0]))   # 14 decades of powers: not the 1.5's
    a = phase + 2 * Rn
    b = a + (L + 5) * Rn
    word = rng.integers(0, K, L).astype(np.uint8)
    if L == 1:
        sym[sym == word[0]] = (word[0] + 1) % K
    metric = R.phase_metric(sym, P, Rn)
    assert int(np.argmax(metric[0])) == phase
    d = handle(Rn, K)
    run = Runner(A, torch, d, sym, P)
    cap = W // Rn + 1

    def go(s, max_errors=0):
        ref_out, ref = R.acquire(s, P, Rn, word, max_errors, metric=metric)
        out, res, _ = run.run(word, max_errors, cap, sym=s)
        check(res, out, ref_out, ref, cap, metric=False)
        return res

    res = go(sym)
    assert res["sync_window"] == -1 and res["n_out"] == 0 and res["n_written"] == 0
    assert res["first_window"] == W
    if Rn > 1:
        other = plant(sym, Rn, (phase + 1) % Rn, word, 0, K, rng)        # window 0 or near it
        assert go(other)["sync_window"] == -1
        assert go(plant(other, Rn, b, word, 0, K, rng))["sync_window"] == b
    two = plant(plant(sym, Rn, b, word, 0, K, rng), Rn, a, word, 0, K, rng)
    assert go(two)["sync_window"] == a
    if L > 1:
        # a worse match first, a perfect one later: the first still wins
        worse = plant(plant(sym, Rn, b, word, 0, K, rng), Rn, a, word, 1, K, rng)
        res = go(worse, 1)
        assert res["sync_window"] == a and res["sync_errors"] == 1
    last = W - 1 - (L - 1) * Rn
    last -= (last - phase) % Rn
    res = go(plant(sym, Rn, last, word, 0, K, rng))
    assert res["sync_window"] == last and res["n_out"] == (1 if last + L * Rn < W else 0)
    # one phase step later the word no longer fits: cut it at the batch's end
    if last + Rn < W:
        s = sym.copy()
        idx = np.arange(last + Rn, W, Rn)
        s[idx] = word[:len(idx)]
        assert go(s, 1 if L > 1 else 0)["sync_window"] == -1


@pytest.mark.parametrize("Rn,K", [(4, 2), (16, 8), (1, 16)])
def test_bytes_above_k(A, torch, handle, Rn, K):
    """Bytes >= K inside sym (0x80, 0xFF, K itself) add nothing to M and match
    no sync symbol; their rows of P are not read out of range (P ends with
    the batch: the last window carries one)."""
    T = A.ACQUIRE_TILE
    W = T + 3 * Rn + 1
    sym, P = make_inputs(W, K, Rn, 3 + K, boost=Rn - 1)
    rng = np.random.default_rng(K)
    bad = rng.choice(W, W // 3, replace=False)
    sym[bad] = np.array([0x80, 0xFF, K], np.uint8)[np.arange(bad.size) % 3]
    sym[W - 1] = 0xFF
    sym[0] = 0x80
    ref_out, ref = R.acquire(sym, P, Rn)
    run = Runner(A, torch, handle(Rn, K), sym, P)
    out, res, _ = run.run(cap=W)
    check(res, out, ref_out, ref, W)
    # all bad on one phase: that phase's metric is exactly 0
    s2 = sym.copy()
    s2[0::Rn] = 0xFF
    ref_out, ref = R.acquire(s2, P, Rn)
    out, res, _ = run.run(cap=W, sym=s2)
    check(res, out, ref_out, ref, W)
    assert res["metric"][0] == 0.0
    # a word whose planted copy holds a byte >= K is a mismatch there
    word = np.arange(6, dtype=np.uint8) % K
    w0 = ref["phase"] + 5 * Rn
    s3 = s2.copy()
    s3[w0:w0 + 6 * Rn:Rn] = word
    s3[w0 + 3 * Rn] = K
    for me in (0, 1):
        ref_out, ref3 = R.acquire(s3, P, Rn, word, me)
        out, res, _ = run.run(word, me, W, sym=s3)
        check(res, out, ref_out, ref3, W)
    if ref3["sync_window"] == w0:        # (the plant may move the phase off the word)
        assert res["sync_errors"] == 1


def test_determinism_and_second_stream(A, torch, handle):
    """Two runs, and a run on a second stream with a workspace of its own,
    give byte-identical *d_result."""
    Rn, K, W = 16, 8, 70001
    sym, P = make_inputs(W, K, Rn, 11, boost=5)
    word = sym[5 + 16 * 40:5 + 16 * 64:16].copy()
    run = Runner(A, torch, handle(Rn, K), sym, P)
    out1, res1, raw1 = run.run(word, 2, 100)
    out2, res2, raw2 = run.run(word, 2, 100)
    side = torch.cuda.Stream()
    other = Runner(A, torch, handle(Rn, K), sym, P)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out3, res3, raw3 = other.run(word, 2, 100, stream=side.cuda_stream)
    assert raw1 == raw2 == raw3
    assert np.array_equal(out1, out2) and np.array_equal(out1, out3)
    ref_out, ref = R.acquire(sym, P, Rn, word, 2)
    check(res1, out1, ref_out, ref, 100)
    assert res1["sync_window"] >= 0


@pytest.mark.parametrize("Rn,K,W", [(4, 2, 4101), (64, 16, 1025), (1, 8, 1), (2, 1, 3)])
def test_guards(A, torch, handle, Rn, K, W):
    """d_out with cap below and above n_out, d_result and d_work between
    poisoned guards; sym and P unchanged; every byte of d_result written."""
    d = handle(Rn, K)
    sym, P = make_inputs(W, K, Rn, 21 + W, boost=Rn - 1)
    ref_out, ref = R.acquire(sym, P, Rn)
    n_out = ref["n_out"]
    # sym and P inside guarded allocations of their own: compared after the runs
    g_sym, chk_sym = G.guarded(torch, W, torch.uint8, LEAD + 3, LEAD, 0xFF)
    g_sym.copy_(torch.from_numpy(sym))
    g_P, chk_P = G.guarded(torch, W * K, torch.float32, G.F32_GUARD + 1, G.F32_GUARD, G.F32_POISON)
    g_P.copy_(torch.from_numpy(P.reshape(-1)))
    raws = []
    for cap in sorted({max(n_out - 1, 0), n_out + 7, 1}):
        for poison in (0xFF, 0x5A):
            # cap 0: no output tensor at all (d_out NULL)
            g_out, chk_out = (G.guarded(torch, cap, torch.uint8, LEAD + 1, LEAD, 0xFF) if cap
                              else (None, lambda written: None))
            g_res, chk_res = G.guarded(torch, RES_BYTES, torch.uint8, LEAD, LEAD, poison)
            g_work, chk_work = G.guarded(torch, A.acquire_workspace_size(d.cfg), torch.uint8, LEAD,
                                         LEAD, poison)
            d.acquire_async(g_sym, g_P, W, None, 0, g_out, g_res, g_work)
            chk_out(written=False)
            chk_res(written=False)
            chk_work(written=False)
            raw = g_res.cpu().numpy().tobytes()
            res = parse(A, raw)
            check(res, g_out.cpu().numpy() if cap else np.zeros(0, np.uint8), ref_out, ref, cap)
            assert res["n_written"] == min(n_out, cap)
            raws.append((cap, raw))
    # the same bytes from either poison: no byte of d_result was left unwritten
    for (c1, r1), (c2, r2) in zip(raws[0::2], raws[1::2]):
        assert c1 == c2 and r1 == r2
    chk_sym(written=False)
    chk_P(written=False)
    assert np.array_equal(g_sym.cpu().numpy(), sym)
    assert np.array_equal(g_P.cpu().numpy().view(np.int32), P.reshape(-1).view(np.int32))


def test_refusals(A, torch, handle):
    """Every DEMOD_BAD_ARG case returns without a launch: the outputs stay poison."""
    lib = A.load_library()
    K, W = 8, 4096
    d = handle(4, K)
    sym, P = make_inputs(W, K, 4, 1)
    d_sym, d_P = torch.from_numpy(sym).cuda(), torch.from_numpy(P).cuda()
    d_out = torch.full((64,), 0xFF, dtype=torch.uint8, device="cuda")
    d_res = torch.full((RES_BYTES,), 0xFF, dtype=torch.uint8, device="cuda")
    d_work = torch.full((A.acquire_workspace_size(d.cfg),), 0xFF, dtype=torch.uint8, device="cuda")
    good = np.arange(8, dtype=np.uint8)

    def call(h, sym_p, mag_p, n_windows, sync, sync_len, max_errors, out_p, cap, res_p, work_p):
        return lib.demod_acquire_async(h, sym_p, mag_p, n_windows, sync, sync_len, max_errors,
                                       out_p, cap, res_p, work_p, None)

    ps, pm, po, pr, pw = (t.data_ptr() for t in (d_sym, d_P, d_out, d_res, d_work))
    sp = good.ctypes.data
    bad_sym = np.array([0, K], np.uint8)
    long_word = np.zeros(65, np.uint8)
    cases = [
        ("W < R", (d._h, ps, pm, 3, None, 0, 0, po, 64, pr, pw)),
        ("sync_len > 64", (d._h, ps, pm, W, long_word.ctypes.data, 65, 0, po, 64, pr, pw)),
        ("sync symbol >= K", (d._h, ps, pm, W, bad_sym.ctypes.data, 2, 0, po, 64, pr, pw)),
        ("max_errors >= sync_len", (d._h, ps, pm, W, sp, 8, 8, po, 64, pr, pw)),
        ("NULL d_symbols", (d._h, None, pm, W, sp, 8, 0, po, 64, pr, pw)),
        ("NULL d_mags", (d._h, ps, None, W, sp, 8, 0, po, 64, pr, pw)),
        ("NULL d_result", (d._h, ps, pm, W, sp, 8, 0, po, 64, None, pw)),
        ("NULL d_work", (d._h, ps, pm, W, sp, 8, 0, po, 64, pr, None)),
        ("NULL d_out with cap", (d._h, ps, pm, W, sp, 8, 0, None, 64, pr, pw)),
        ("NULL sync with sync_len", (d._h, ps, pm, W, None, 8, 0, po, 64, pr, pw)),
    ]
    # hop does not divide n; more than 64 phases
    others = [A.Demodulator(n=1024, hop=384, freqs=(1500.0, 3000.0)),
              A.Demodulator(n=1024, hop=8, freqs=(1500.0, 3000.0))]
    try:
        cases.append(("n % hop != 0", (others[0]._h, ps, pm, W, None, 0, 0, po, 64, pr, pw)))
        cases.append(("R > 64", (others[1]._h, ps, pm, W, None, 0, 0, po, 64, pr, pw)))
        for what, args in cases:
            assert call(*args) == A.DEMOD_BAD_ARG, what
        for dd in others:
            with pytest.raises(A.DemodError) as e:
                dd.acquire(np.zeros(4096, np.int16))
            assert e.value.code == A.DEMOD_BAD_ARG
    finally:
        for dd in others:
            dd.close()
    # the Python mirror's own checks (before any pointer reaches the library)
    for kw in (dict(d_sym=d_sym[:W - 1]), dict(d_mag=d_P.reshape(-1)[:W * K - 1]),
               dict(d_result=d_res[:RES_BYTES - 1]), dict(d_work=d_work[:-1]),
               dict(d_sym=d_sym.cpu()), dict(d_result=d_res.to(torch.int16))):
        a = dict(d_sym=d_sym, d_mag=d_P, d_result=d_res, d_work=d_work)
        a.update(kw)
        with pytest.raises(A.DemodError) as e:
            d.acquire_async(a["d_sym"], a["d_mag"], W, good, 0, d_out, a["d_result"], a["d_work"])
        assert e.value.code == A.DEMOD_BAD_ARG
    torch.cuda.synchronize()
    for t in (d_out, d_res, d_work):
        assert bool((t == 0xFF).all()), "a refused call wrote"
    # and the same call, legal, runs
    d.acquire_async(d_sym, d_P, W, good, 0, d_out, d_res, d_work)
    torch.cuda.synchronize()
    assert parse(A, d_res.cpu().numpy().tobytes())["phases"] == 4


# ---- end to end --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case_reference(name, tau):
    """(x, truth, oracle sym, oracle P): computed once per case and tau."""
    from oracle import oracle as O
    freqs, n, hop = R.CASES[name][:3]
    x, truth = R.case_stream(O, name, tau)
    sym, P = O.goertzel(x, freqs, n, hop)
    return x, truth, sym, P


def check_e2e(res, out, name, tau, W):
    freqs, n, hop = R.CASES[name][:3]
    Rn = n // hop
    x, truth, sym, P = case_reference(name, tau)
    assert W == len(sym)
    word = truth[5:29]
    ref_out, ref = R.acquire(sym, P, Rn, word, 0)
    Mr = ref["metric"]
    s = np.sort(Mr)
    assert s[-1] - s[-2] > 4e-5 * s[-1]                 # the reference's margin, first
    assert res["phase"] == ref["phase"] == (tau + hop // 2) // hop
    J = ref["per_phase"]
    err = np.abs(res["metric"] - Mr)
    print(f"case {name} tau {tau}: max |M - M_ref| / M_ref {float((err / Mr).max()):.3e}")
    assert (err <= MAG_TOL * Mr + J * EPS * Mr).all()
    for f in ("sync_window", "sync_errors", "first_window", "n_out", "per_phase", "phases"):
        assert res[f] == ref[f], f
    assert res["n_written"] == ref["n_out"] == len(out) > 0
    assert np.array_equal(out, ref_out)
    assert np.array_equal(out, truth[29:29 + len(out)])   # the transmitted symbols after the word


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_end_to_end(A, torch, name):
    """batch + acquire_async, acquire from a host array and from a device
    tensor: cases A-D, each tau."""
    freqs, n, hop = R.CASES[name][:3]
    Rn = n // hop
    with A.Demodulator(n=n, hop=hop, freqs=freqs) as d:
        d_work = torch.empty(A.acquire_workspace_size(d.cfg), dtype=torch.uint8, device="cuda")
        for tau, _ in R.case_taus(n, hop):
            x, truth, sym, P = case_reference(name, tau)
            W = len(sym)
            word = truth[5:29]
            d_pcm = torch.from_numpy(x).cuda()
            d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
            d_mag = torch.empty(W * d.k, dtype=torch.float32, device="cuda")
            d_out = torch.full((W // Rn + 1,), 0xFF, dtype=torch.uint8, device="cuda")
            d_res = torch.full((RES_BYTES,), 0xFF, dtype=torch.uint8, device="cuda")
            assert d.batch_async(d_pcm, W, d_sym, d_mag) == W
            d.acquire_async(d_sym, d_mag, W, word, 0, d_out, d_res, d_work)
            torch.cuda.synchronize()
            res = parse(A, d_res.cpu().numpy().tobytes())
            check_e2e(res, d_out.cpu().numpy()[:res["n_written"]], name, tau, W)
            out_h, res_h = d.acquire(x, sync=word)
            check_e2e(res_h, out_h, name, tau, W)
            out_d, res_d = d.acquire(d_pcm, sync=word)
            check_e2e(res_d, out_d, name, tau, W)
            # one handle, one input: the three paths agree bit for bit
            for f in res:
                assert np.array_equal(res[f], res_h[f]) and np.array_equal(res[f], res_d[f]), f
            # a short cap cuts the copy, not the count
            out_c, res_c = d.acquire(x, sync=word, cap=3)
            assert res_c["n_out"] == res["n_out"] and res_c["n_written"] == 3
            assert np.array_equal(out_c, out_h[:3])


def test_capture_and_replay(A, torch):
    """demod_batch_async + demod_acquire_async in one linear graph on a side
    stream, replayed on two contents at different tau: each replay's result is
    the eager result for that content."""
    name = "A"
    freqs, n, hop = R.CASES[name][:3]
    Rn = n // hop
    taus = (256, 576)
    refs = [case_reference(name, t) for t in taus]
    W = min(len(r[2]) for r in refs)
    need = (W - 1) * hop + n
    word = refs[0][1][5:29]
    with A.Demodulator(n=n, hop=hop, freqs=freqs) as d:
        d_pcm = torch.zeros(need, dtype=torch.int16, device="cuda")
        d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
        d_mag = torch.empty(W * d.k, dtype=torch.float32, device="cuda")
        d_out = torch.empty(W // Rn + 1, dtype=torch.uint8, device="cuda")
        d_res = torch.empty(RES_BYTES, dtype=torch.uint8, device="cuda")
        d_work = torch.empty(A.acquire_workspace_size(d.cfg), dtype=torch.uint8, device="cuda")

        def step(stream):
            d.batch_async(d_pcm, W, d_sym, d_mag, stream=stream)
            d.acquire_async(d_sym, d_mag, W, word, 0, d_out, d_res, d_work, stream=stream)

        def results():
            torch.cuda.synchronize()
            raw = d_res.cpu().numpy().tobytes()
            return raw, d_out.cpu().numpy()[:parse(A, raw)["n_written"]].copy()

        side = torch.cuda.Stream()
        eager = []
        with torch.cuda.stream(side):
            for x, *_ in refs:                            # eager calls of the shape first
                d_pcm.copy_(torch.from_numpy(x[:need]))
                step(side.cuda_stream)
                side.synchronize()
                eager.append(results())
        assert eager[0][0] != eager[1][0]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step(torch.cuda.current_stream().cuda_stream)
        for rep in range(2):
            for i, (x, *_) in enumerate(refs):
                d_pcm.copy_(torch.from_numpy(x[:need]))
                d_res.fill_(0xFF)
                d_out.fill_(0xFF)
                torch.cuda.synchronize()
                g.replay()
                raw, out = results()
                assert raw == eager[i][0] and np.array_equal(out, eager[i][1]), (rep, i)
        # and the eager results are right: phase tau / hop (or the nearer), the word found
        for (raw, out), tau, (x, truth, sym, P) in zip(eager, taus, refs):
            res = parse(A, raw)
            ref_out, ref = R.acquire(sym[:W], P[:W], Rn, word, 0)
            assert res["phase"] == ref["phase"] == (tau + hop // 2) // hop
            assert res["sync_window"] == ref["sync_window"] and res["n_out"] == ref["n_out"]
            assert np.array_equal(out, ref_out)
