"""The segmented frame scan without a GPU: the ABI (exports, workspace size,
refusals that need no device), the reference of tests/frames_segments_ref.py
against a brute-force loop on random segment tables, and the slip scenario on
the oracle: a stream that loses n / 2 samples before its third frame loses
frames as one batch and keeps all five as two segments."""
import ctypes

import numpy as np
import pytest

import acquire_ref as R
import acquire_segments_ref as SR
import frames_ref as F
import frames_segments_ref as FS
from test_frames_cpu import brute

EXPORTS = ("demod_frames_segments_workspace_size", "demod_frames_segments_async", "demod_frames_segments")


def test_exports(A):
    lib = A.load_library()
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in A.header_exports()
    for name in ("frames_segments_workspace_size",):
        assert callable(getattr(A, name))
    for name in ("frames_segments", "frames_segments_async"):
        assert callable(getattr(A.Demodulator, name))
    assert FS.TILE == A.ACQUIRE_TILE


def test_entry_points_refuse_null(A):
    lib = A.load_library()
    res = A.DemodFramesResult()
    first = np.zeros(1, np.uint64)
    count = np.full(1, 8, np.uint32)
    word = np.zeros(2, np.uint8)
    pcm = np.zeros(4096 + 8, np.int16)
    pcm = pcm[(-pcm.ctypes.data % 16) // 2:][:4096]
    assert lib.demod_frames_segments_async(None, None, None, 8, None, None, 1, None, 0, 0, 0, None, None,
                                           None, 0, None, None, 0, None) == A.DEMOD_BAD_ARG
    # non-NULL pointers everywhere: the handle alone is missing
    p = first.ctypes.data
    assert lib.demod_frames_segments_async(None, p, p, 8, p, count.ctypes.data, 1, word.ctypes.data, 2, 0,
                                           0, p, None, None, 1, p, p, 1 << 20, None) == A.DEMOD_BAD_ARG
    assert lib.demod_frames_segments(None, pcm.ctypes.data, 1, first.ctypes.data, count.ctypes.data, 1,
                                     word.ctypes.data, 2, 0, 0, None, None, None, 0,
                                     ctypes.byref(res)) == A.DEMOD_BAD_ARG
    assert lib.demod_frames_segments(None, None, 1, None, None, 1, None, 0, 0, 0, None, None, None, 0,
                                     None) == A.DEMOD_BAD_ARG


def test_workspace_size(A):
    """0 for bad configurations, max_segments 0 or > 65536 and 2^31 windows;
    monotone in both arguments; equal to the documented formula."""
    lib = A.load_library()
    for n, hop in [(1024, 1024), (1024, 256), (1024, 64), (256, 64), (512, 8)]:
        cfg = A.make_cfg(n=n, hop=hop)
        Rn = n // hop
        segs = (1, 2, 9, 1024, 1025, 65536)
        wins = (0, 1, 1023, 1024, 1025, 100000, 4194301, 0x7FFFFFFF)
        size = {(s, w): A.frames_segments_workspace_size(cfg, s, w) for s in segs for w in wins}
        for (s, w), v in size.items():
            assert v % 8 == 0 and v == FS.workspace_size(Rn, s, w), (n, hop, s, w)
            # exactly the tiles it promises, and not one more
            assert FS.budget_of(v, Rn, s) == SR.budget_for(s, w)
            assert FS.budget_of(v - 1, Rn, s) == SR.budget_for(s, w) - 1
        for s in segs:                                   # monotone in the windows
            assert all(size[s, a] <= size[s, b] for a, b in zip(wins, wins[1:]))
        for w in wins:                                   # and in the segments
            assert all(size[a, w] < size[b, w] for a, b in zip(segs, segs[1:]))
        for s, w in [(0, 1024), (65537, 1024), (1, 0x80000000)]:
            assert lib.demod_frames_segments_workspace_size(ctypes.byref(cfg), s, w) == 0
            with pytest.raises(A.DemodError) as e:
                A.frames_segments_workspace_size(cfg, s, w)
            assert e.value.code == A.DEMOD_BAD_ARG
    # hop does not divide n; more than 64 phases; an invalid configuration
    for n, hop in [(1024, 384), (1024, 8), (4096, 32), (1000, 250)]:
        cfg = A.make_cfg(n=n, hop=hop)
        assert lib.demod_frames_segments_workspace_size(ctypes.byref(cfg), 4, 4096) == 0
    assert lib.demod_frames_segments_workspace_size(None, 4, 4096) == 0


def test_budget_rule():
    """budget_of is the largest B whose words fit, for odd B and R = 1 too (the
    4-byte arrays are padded to 8)."""
    for Rn in (1, 2, 4, 64):
        for S in (1, 3, 1025):
            for B in range(0, 9):
                need = FS.header_bytes(S) + FS.tiles_bytes(B, Rn)
                assert FS.budget_of(need, Rn, S) == B
                assert FS.budget_of(need + 7, Rn, S) == B
                if B:
                    assert FS.budget_of(need - 1, Rn, S) == B - 1
    assert FS.budget_of(0, 4, 9) == 0


@pytest.mark.parametrize("Rn", [1, 4])
@pytest.mark.parametrize("K", [2, 8])
def test_reference_against_brute_force(Rn, K):
    """Random tables (overlapping, reversed, out-of-range and short segments)
    with a 16-window tile and a random budget, against a loop that applies the
    clamp, the short rule and the budget itself and scans each slice with
    test_frames_cpu.brute."""
    rng = np.random.default_rng(1000 * Rn + K)
    tile = 16
    seen = dict(hits=0, tail=0, short=0, dropped=0, clamped=0, overlap=0)
    for trial in range(25):
        Wb = int(rng.integers(40, 300))
        L = int(rng.integers(1, 4))
        N = int(rng.integers(0, 5))
        me = int(rng.integers(0, L))
        sym = rng.integers(0, K, Wb).astype(np.uint8)
        sym[rng.integers(0, Wb, Wb // 10)] = 0xFF
        P = rng.integers(1, 1 << 20, (Wb, K)).astype(np.float64)    # dyadic: every sum exact
        sync = rng.integers(0, K, L).astype(np.uint8)
        S = int(rng.integers(1, 9))
        first = [int(v) for v in rng.integers(0, Wb, S)]
        count = [int(v) for v in rng.integers(0, Wb // 2, S)]
        first[0], count[0] = 0, Wb                                   # the whole batch: overlaps every other
        if S > 2:
            first[1], count[1] = Wb + 7, 5                           # past the batch
            first[2], count[2] = Wb - 3 * Rn, 0xFFFFFFFF             # runs out of it
        if S > 3:
            count[3] = Rn - 1                                        # short
        if trial % 2:
            first, count = first[::-1], count[::-1]                  # reversed
        budget = None if trial % 3 == 0 else int(rng.integers(1, 2 * -(-Wb // tile)))
        got = FS.frames_segments(sym, P, Rn, first, count, sync, me, N, budget=budget, tile=tile)
        used = 0
        for s, (f, c) in enumerate(zip(first, count)):
            f2 = min(f, Wb)
            c2 = min(c, Wb - f2)
            seen["clamped"] += (f2, c2) != (f, c)
            tiles = -(-c2 // tile) if c2 >= Rn else 0
            used += tiles
            hits, payload, packed, res = got[s]
            if tiles == 0 or (budget is not None and used > budget):
                seen["short" if tiles == 0 else "dropped"] += 1
                assert res["phases"] == Rn and res["phase"] == 0 and res["per_phase"] == 0
                assert not res["metric"].any() and len(res["metric"]) == Rn
                assert res["n_hits"] == res["n_written"] == 0
                assert (res["tail_window"], res["tail_errors"]) == (-1, 0)
                assert len(hits) == 0 and payload.shape == (0, N)
                continue
            phase, bh, bt = brute(sym[f2:f2 + c2], P[f2:f2 + c2], Rn, sync, me, N)
            assert res["phase"] == phase and res["per_phase"] == c2 // Rn
            assert res["n_hits"] == len(bh) == res["n_written"]
            assert hits["window"].tolist() == [h[0] for h in bh]
            assert hits["errors"].tolist() == [h[1] for h in bh]
            assert payload.tolist() == [h[2] for h in bh] or (N == 0 and payload.shape == (len(bh), 0))
            assert (res["tail_window"], res["tail_errors"]) == (bt if bt else (-1, 0))
            assert np.array_equal(packed, F.pack(payload, F.bits_per_symbol(K)))
            seen["hits"] += len(bh)
            seen["tail"] += bt is not None
            seen["overlap"] += s > 0 and c2 > 0
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("name,freqs", [("2-FSK", F.FSK2), ("8-FSK", F.FSK8)])
def test_slip_on_the_oracle(O, name, freqs):
    """n / 2 samples deleted two symbols before the third of the five frames
    (n 1024, hop 256, max_errors 1), on the oracle's double sliding powers: the
    whole-batch reference returns fewer than five frames; the same batch as two
    segments split at the slip returns all five with exact payloads."""
    n, hop, Rn = 1024, 256, 4
    x, word, payloads, cut, rel = FS.slip_stream(freqs, n, hop)
    sym, P = O.goertzel(x, freqs, n, hop)
    W = len(sym)
    w_hits, w_pay, _, w_res = F.frames(sym, P, Rn, word, 1, F.FRAME_N)
    print(f"{name}: whole batch of {W}: phase {w_res['phase']} margin {R.margin(w_res['metric']):.4f} "
          f"hits {w_hits['window'].tolist()}")
    assert w_res["n_hits"] < F.FRAME_COUNT
    (h1, p1, k1, r1), (h2, p2, k2, r2) = FS.frames_segments(sym, P, Rn, [0, cut], [cut, W - cut], word, 1,
                                                            F.FRAME_N)
    print(f"{name}: two segments cut at {cut}: phases {r1['phase']} {r2['phase']} margins "
          f"{R.margin(r1['metric']):.4f} {R.margin(r2['metric']):.4f} hits {h1['window'].tolist()} "
          f"{h2['window'].tolist()}")
    assert (r1["phase"], r2["phase"]) == (0, 2)
    assert h1["window"].tolist() + h2["window"].tolist() == rel
    assert r1["n_hits"] + r2["n_hits"] == F.FRAME_COUNT and r1["n_hits"] == 2
    assert r1["tail_window"] == -1 and r2["tail_window"] == -1
    assert np.array_equal(np.concatenate([p1, p2]), payloads)
    assert np.array_equal(np.concatenate([k1, k2]), F.pack(payloads, F.bits_per_symbol(len(freqs))))
