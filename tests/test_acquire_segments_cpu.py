"""Segmented acquisition without a GPU: the ABI (exports, workspace size,
refusals that need no device), demod_segments_layout against a restatement of
stream_stage.h run_layout, and the slip scenario on the oracle: a stream that
loses hop .. (R - 1) hop samples in its middle is acquired wrongly as one batch
and rightly as two segments (tests/acquire_segments_ref.py)."""
import ctypes

import numpy as np
import pytest

import acquire_ref as R
import acquire_segments_ref as SR

EXPORTS = ("demod_acquire_segments_workspace_size", "demod_acquire_segments_async",
           "demod_acquire_segments", "demod_segments_layout")


def test_exports(A):
    lib = A.load_library()
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in A.header_exports()
    hdr = open(A.HEADER_PATH).read()
    assert "#define DEMOD_MAX_SEGMENTS %d" % A.DEMOD_MAX_SEGMENTS in hdr
    assert A.DEMOD_MAX_SEGMENTS == 65536 and SR.TILE == A.ACQUIRE_TILE


def test_workspace_size(A):
    lib = A.load_library()
    for n, hop in [(1024, 1024), (1024, 256), (1024, 64), (256, 64), (512, 8)]:
        cfg = A.make_cfg(n=n, hop=hop)
        Rn = n // hop
        segs = (1, 2, 9, 1024, 1025, 65536)
        wins = (0, 1, 1023, 1024, 1025, 100000, 4194301, 0x7FFFFFFF)
        size = {(s, w): A.acquire_segments_workspace_size(cfg, s, w) for s in segs for w in wins}
        for (s, w), v in size.items():
            assert v > 0 and v % 8 == 0
            # room for the tiles it promises, one partial and one word per phase each
            assert v >= 16 * Rn * SR.budget_for(s, w)
        for s in segs:                                   # monotone in the windows
            assert all(size[s, a] <= size[s, b] for a, b in zip(wins, wins[1:]))
        for w in wins:                                   # and in the segments
            assert all(size[a, w] < size[b, w] for a, b in zip(segs, segs[1:]))
        # one more tile of windows is one more tile of words, exactly
        assert size[9, 1025] - size[9, 1024] == 16 * Rn
        for s, w in [(0, 1024), (65537, 1024), (1, 0x80000000)]:
            assert lib.demod_acquire_segments_workspace_size(ctypes.byref(cfg), s, w) == 0
            with pytest.raises(A.DemodError) as e:
                A.acquire_segments_workspace_size(cfg, s, w)
            assert e.value.code == A.DEMOD_BAD_ARG
    # hop does not divide n; more than 64 phases; an invalid configuration
    for n, hop in [(1024, 384), (1024, 8), (4096, 32), (1000, 250)]:
        cfg = A.make_cfg(n=n, hop=hop)
        assert lib.demod_acquire_segments_workspace_size(ctypes.byref(cfg), 4, 4096) == 0
    assert lib.demod_acquire_segments_workspace_size(None, 4, 4096) == 0


def test_entry_points_refuse_null_handle(A):
    lib = A.load_library()
    res = A.DemodAcquireResult()
    first = np.zeros(1, np.uint64)
    count = np.full(1, 8, np.uint32)
    pcm = np.zeros(4096 + 8, np.int16)
    pcm = pcm[(-pcm.ctypes.data % 16) // 2:][:4096]
    assert lib.demod_acquire_segments_async(None, None, None, 8, None, None, 1, None, 0, 0, None, 0,
                                            None, None, 0, None) == A.DEMOD_BAD_ARG
    # non-NULL pointers everywhere: the handle alone is missing
    p = first.ctypes.data
    assert lib.demod_acquire_segments_async(None, p, p, 8, p, count.ctypes.data, 1, None, 0, 0, None, 0,
                                            p, p, 1 << 20, None) == A.DEMOD_BAD_ARG
    assert lib.demod_acquire_segments(None, pcm.ctypes.data, 1, first.ctypes.data, count.ctypes.data, 1,
                                      None, 0, 0, None, 0, ctypes.byref(res)) == A.DEMOD_BAD_ARG


def run_layout(n, hop, lengths):
    """stream_stage.h run_layout, restated: a run of w complete windows is
    (w - 1) hop + n samples and takes ceil of that over hop batch windows."""
    first, count, Wb = [], [], 0
    for total in lengths:
        w = 0 if total < n else (total - n) // hop + 1
        first.append(Wb)
        count.append(w)
        if w:
            Wb += -(-((w - 1) * hop + n) // hop)
    return first, count, Wb


def test_segments_layout(A):
    rng = np.random.default_rng(0x5E6)
    seen = set()
    for it in range(200):
        n = int(rng.choice([64, 256, 1024, 4096]))
        hop = n if it % 4 == 0 else int(rng.choice([h for h in (8, 16, 64, 256, 1024, 4096) if h <= n]))
        S = int(rng.integers(1, 40))
        lengths = rng.integers(0, 6 * n, S)
        lengths[rng.integers(0, S)] = n                       # exactly one window
        lengths[rng.integers(0, S)] = int(rng.integers(0, n))  # none
        if it % 3 == 0:
            lengths[rng.integers(0, S)] = n + hop * int(rng.integers(0, 50)) + int(rng.integers(0, hop))
        cfg = A.make_cfg(n=n, hop=hop)
        first, count, Wb = A.segments_layout(cfg, lengths)
        f, c, W = run_layout(n, hop, [int(v) for v in lengths])
        assert first.dtype == np.uint64 and count.dtype == np.uint32
        assert first.tolist() == f and count.tolist() == c and Wb == W, (n, hop, lengths)
        # the runs do not overlap and the gap between two is the straddling windows
        for s in range(S - 1):
            if c[s]:
                assert f[s + 1] - (f[s] + c[s]) == (n // hop - 1 if n % hop == 0 else
                                                    -(-((c[s] - 1) * hop + n) // hop) - c[s])
        seen |= {("hop=n", hop == n), ("short", bool((lengths < n).any())), ("one", bool((lengths == n).any()))}
    assert {("hop=n", True), ("hop=n", False), ("short", True), ("one", True)} <= seen
    lib = A.load_library()
    cfg = A.make_cfg(n=1024, hop=256)
    lens = np.array([5000, 100], np.uint64)
    W = ctypes.c_size_t(0)
    # the tables are optional; the counts are not
    assert lib.demod_segments_layout(ctypes.byref(cfg), 2, lens.ctypes.data, None, None,
                                     ctypes.byref(W)) == A.DEMOD_OK
    assert W.value == run_layout(1024, 256, [5000, 100])[2]
    for args in [(None, 2, lens.ctypes.data, None, None, ctypes.byref(W)),
                 (ctypes.byref(cfg), 0, lens.ctypes.data, None, None, ctypes.byref(W)),
                 (ctypes.byref(cfg), 65537, lens.ctypes.data, None, None, ctypes.byref(W)),
                 (ctypes.byref(cfg), 2, None, None, None, ctypes.byref(W)),
                 (ctypes.byref(cfg), 2, lens.ctypes.data, None, None, None)]:
        assert lib.demod_segments_layout(*args) == A.DEMOD_BAD_ARG
    huge = np.array([1 << 40, 100], np.uint64)                # a batch of 2^31 windows or more
    assert lib.demod_segments_layout(ctypes.byref(cfg), 2, huge.ctypes.data, None, None,
                                     ctypes.byref(W)) == A.DEMOD_BAD_ARG
    bad = A.make_cfg(n=1000, hop=250)
    assert lib.demod_segments_layout(ctypes.byref(bad), 2, lens.ctypes.data, None, None,
                                     ctypes.byref(W)) == A.DEMOD_BAD_ARG


def test_reference_rules():
    """The clamp, the short-segment rule and the tile budget of the reference."""
    K, Rn, Wb = 2, 4, 40
    rng = np.random.default_rng(3)
    sym = rng.integers(0, K, Wb).astype(np.uint8)
    P = rng.uniform(1.0, 2.0, (Wb, K))
    first = [0, 50, 36, 8, 30]
    count = [8, 4, 0xFFFFFFFF, 3, 12]
    got = SR.acquire_segments(sym, P, Rn, first, count)
    out, res = R.acquire(sym[:8], P[:8], Rn)
    assert got[0][1]["phase"] == res["phase"] and np.array_equal(got[0][0], out)
    assert got[1][1] == {**SR.short_result(Rn, 0), "metric": got[1][1]["metric"]}   # first >= Wb
    assert got[1][1]["first_window"] == 0 and not got[1][1]["metric"].any()
    assert got[2][1]["per_phase"] == 1 and got[2][1]["n_out"] == 1                   # 4 windows left
    assert got[3][1]["first_window"] == 3 and got[3][1]["n_out"] == 0                # count < R
    assert got[4][1]["per_phase"] == 2                                               # 10 windows left
    # budget 2 with one-window tiles of 4: segment 0 takes both
    got = SR.acquire_segments(sym, P, Rn, [0, 8, 16], [8, 4, 2], budget=2, tile=4)
    assert got[0][1]["per_phase"] == 2 and got[1][1]["per_phase"] == 0 and got[1][1]["first_window"] == 4
    assert got[2][1]["first_window"] == 2


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_slip_on_the_oracle(O, name):
    """Samples deleted in mid-stream: as one batch the phase margin collapses
    and the symbols after the slip are read at the wrong phase; as two
    segments split at the slip each side has its own phase (0, and (n - drop) /
    hop) with the reference's margin, and the second's symbols are the truth."""
    freqs, n, hop, ns = R.CASES[name][:4]
    Rn = n // hop
    for drop in SR.slip_drops(n, hop):
        x, truth, cut, phase2 = SR.slip_stream(O, name, drop)
        sym, P = O.goertzel(x, freqs, n, hop)
        W = len(sym)
        (out1, res1), (out2, res2) = SR.acquire_segments(sym, P, Rn, [0, cut], [cut, W - cut])
        m1, m2 = R.margin(res1["metric"]), R.margin(res2["metric"])
        _, whole = R.acquire(sym, P, Rn)
        print(f"case {name} drop {drop}: cut {cut} of {W}, phases {res1['phase']} {res2['phase']} "
              f"margins {m1:.4f} {m2:.4f}, whole-batch margin {R.margin(whole['metric']):.4f}")
        assert res1["phase"] == 0 and res2["phase"] == phase2 == ((n - drop) % n) // hop
        assert m1 > 4e-5 and m2 > 4e-5
        # the second segment: every symbol after the shortened one, up to a cut last symbol
        want = truth[ns // 2 + 1:]
        assert res2["first_window"] == phase2 and res2["n_out"] == len(out2) > 0
        assert np.array_equal(out2, want[:len(out2)]) and len(want) - len(out2) <= 1
        # the first: the symbols before the slip
        assert np.array_equal(out1, truth[:len(out1)]) and len(out1) == ns // 2
        # as one batch there is one phase for both sides: the margin collapses (0.41 .. 0.44,
        # B 0.12, without a slip) and the windows after the slip hold n - drop samples of
        # symbol i and drop of symbol i + 1. From drop = n / 2 on they no longer decide
        # symbol i (SR.whole_batch_misreads); below it they still do, on a thinner margin.
        assert whole["phase"] != phase2 and R.margin(whole["metric"]) < 0.05
        bad = SR.whole_batch_misreads(sym[whole["phase"]::Rn], truth, ns)
        print(f"    whole batch: phase {whole['phase']}, {bad} symbols after the slip misread")
        assert bad > 0 or 2 * drop < n
