"""The frame scan without a GPU: the ABI (exports, struct layouts, workspace
size), the reference of tests/frames_ref.py against a brute-force loop and
against demod_pack_symbols, and the reference on the oracle's double
sliding-window powers of a five-frame stream."""
import ctypes

import numpy as np
import pytest

import acquire_ref as R
import frames_ref as F


def test_exports_and_structs(A):
    lib = A.load_library()
    for name in ("demod_frames_workspace_size", "demod_frames_async", "demod_frames"):
        assert hasattr(lib, name), name
        assert name in A.header_exports()
    H, T = A.DemodFrameHit, A.DemodFramesResult
    assert ctypes.sizeof(H) == 16 and (H.window.offset, H.errors.offset, H.reserved.offset) == (0, 8, 12)
    assert A.FRAME_HIT_DTYPE.itemsize == 16 and A.FRAME_HIT_DTYPE == F.HIT_DTYPE
    assert ctypes.sizeof(T) == F.RESULT_DTYPE.itemsize and [f for f, _ in T._fields_] == list(F.RESULT_DTYPE.names)
    for f in F.RESULT_DTYPE.names:                                  # every field where the tests' one dtype has it
        at, size = F.RESULT_DTYPE.fields[f][1], F.RESULT_DTYPE[f].itemsize
        assert (getattr(T, f).offset, getattr(T, f).size) == (at, size), f
    A_T = A.DemodAcquireResult
    for f in ("metric", "phases", "phase", "per_phase"):            # as demod_acquire_result_t
        assert getattr(T, f).offset == getattr(A_T, f).offset
    assert lib.demod_frames_async(None, None, None, 4, None, 0, 0, 0, None, None, None, 0, None, None,
                                  0, None) == A.DEMOD_BAD_ARG
    res = T()
    assert lib.demod_frames(None, None, 4, None, 0, 0, 0, None, None, None, 0,
                            ctypes.byref(res)) == A.DEMOD_BAD_ARG


def test_workspace_size(A):
    """0 for a bad configuration and for 2^31 windows; monotone in max_windows;
    covers the layout include/demod.h documents: 16 * 1024 * R bytes of block
    words, 4 bytes a tile, 4 R bytes a tile."""
    lib = A.load_library()
    T = A.ACQUIRE_TILE
    for n, hop in [(1024, 1024), (1024, 256), (512, 8), (256, 64)]:
        cfg = A.make_cfg(n=n, hop=hop)
        Rn = n // hop
        last = 0
        for W in (0, 1, Rn, T - 1, T, T + 1, 4 * T + 5, 70001, 4194301, 2 ** 31 - 1):
            s = A.frames_workspace_size(cfg, W)
            tiles = -(-W // T)
            assert s % 8 == 0 and s >= 16 * 1024 * Rn + 4 * tiles + 4 * tiles * Rn
            assert s <= 16 * 1024 * Rn + 4 * tiles + 4 * tiles * Rn + 8      # and no more than it says
            assert s >= last
            last = s
        assert lib.demod_frames_workspace_size(ctypes.byref(cfg), 2 ** 31) == 0
        with pytest.raises(A.DemodError) as e:
            A.frames_workspace_size(cfg, 2 ** 31)
        assert e.value.code == A.DEMOD_BAD_ARG
    # hop does not divide n; more than 64 phases; an invalid configuration
    for n, hop in [(1024, 384), (1024, 8), (1000, 250)]:
        cfg = A.make_cfg(n=n, hop=hop)
        assert lib.demod_frames_workspace_size(ctypes.byref(cfg), 4096) == 0
        with pytest.raises(A.DemodError):
            A.frames_workspace_size(cfg, 4096)
    assert lib.demod_frames_workspace_size(None, 4096) == 0


@pytest.mark.parametrize("K", [1, 2, 3, 8, 16])
def test_pack_against_the_library(A, K):
    """frames_ref.pack is demod_pack_symbols, bytes >= K (masked) included."""
    rng = np.random.default_rng(K)
    bits = F.bits_per_symbol(K)
    assert bits == A.bits_per_symbol(K)
    for N in (0, 1, 7, 8, 9, 64, 300):
        rows = rng.integers(0, 256, (5, N)).astype(np.uint8)
        got = F.pack(rows, bits)
        assert got.shape == (5, (N * bits + 7) // 8)
        for i in range(5):
            assert bytes(got[i]) == A.pack_symbols(rows[i], bits)


def brute(sym, P, Rn, sync, max_errors, N):
    W, K = len(sym), P.shape[1]
    M = [0.0] * Rn
    for r in range(Rn):
        M[r] = sum(float(P[j * Rn + r][sym[j * Rn + r]]) for j in range(W // Rn) if sym[j * Rn + r] < K)
    phase = max(range(Rn), key=lambda r: (M[r], -r))
    L = len(sync)
    hits, tail = [], None
    for w in range(phase, W, Rn):
        if w + (L - 1) * Rn >= W:
            break
        err = sum(int(sym[w + i * Rn]) != int(sync[i]) for i in range(L))
        if err > max_errors:
            continue
        if w + (L + N - 1) * Rn < W:
            hits.append((w, err, [int(sym[w + (L + j) * Rn]) for j in range(N)]))
        elif tail is None:
            tail = (w, err)
    return phase, hits, tail


@pytest.mark.parametrize("Rn", [1, 4])
@pytest.mark.parametrize("K", [2, 8])
def test_reference_against_brute_force(Rn, K):
    rng = np.random.default_rng(100 * Rn + K)
    seen_hits = seen_tail = 0
    for trial in range(30):
        W = int(rng.integers(Rn, 400))
        L = int(rng.integers(1, 5))
        N = int(rng.integers(0, 6))
        me = int(rng.integers(0, L))
        sym = rng.integers(0, K, W).astype(np.uint8)
        sym[rng.integers(0, W, W // 10)] = 0xFF                 # bytes >= K
        # powers on a dyadic grid: every sum is exact, the brute loop's plain sum included
        P = rng.integers(1, 1 << 20, (W, K)).astype(np.float64)
        sync = rng.integers(0, K, L).astype(np.uint8)
        hits, payload, packed, res = F.frames(sym, P, Rn, sync, me, N)
        phase, bh, bt = brute(sym, P, Rn, sync, me, N)
        assert res["phase"] == phase and res["n_hits"] == len(bh) == res["n_written"]
        assert hits["window"].tolist() == [h[0] for h in bh]
        assert hits["errors"].tolist() == [h[1] for h in bh]
        assert payload.tolist() == [h[2] for h in bh] or (N == 0 and payload.shape == (len(bh), 0))
        assert (res["tail_window"], res["tail_errors"]) == (bt if bt else (-1, 0))
        assert np.array_equal(packed, F.pack(payload, F.bits_per_symbol(K)))
        cut = F.frames(sym, P, Rn, sync, me, N, max_frames=1)
        assert cut[3]["n_hits"] == len(bh) and cut[3]["n_written"] == min(1, len(bh))
        assert np.array_equal(cut[0], hits[:1])
        seen_hits += len(bh)
        seen_tail += bt is not None
    assert seen_hits > 30 and seen_tail > 0


def test_reference_on_the_oracle(O):
    """Five frames of a 24-symbol word and 64 payload symbols in acquire_ref's
    case A plan, a symbol boundary at tau: with max_errors = 1 the reference on
    the oracle's double powers returns exactly the planted windows and payloads."""
    freqs, n, hop = R.CASES["A"][:3]
    assert freqs == F.FSK2 and (n, hop, R.CASES["A"][4]) == (1024, 256, 400)
    Rn = n // hop
    for tau in F.FRAME_TAUS:
        x, word, payloads, windows = F.frame_stream(freqs, tau)
        sym, P = O.goertzel(x, freqs, n, hop)
        hits, payload, packed, res = F.frames(sym, P, Rn, word, 1, F.FRAME_N)
        print(f"tau {tau}: W {len(sym)} phase {res['phase']} margin {R.margin(res['metric']):.4f} "
              f"hits {hits['window'].tolist()} errors {hits['errors'].tolist()} tail {res['tail_window']}")
        assert res["phase"] == (tau + hop // 2) // hop
        assert hits["window"].tolist() == windows.tolist()       # the fixture's condition
        assert res["n_hits"] == F.FRAME_COUNT and res["tail_window"] == -1
        assert (hits["errors"] == 0).all()
        assert np.array_equal(payload, payloads)
        assert np.array_equal(packed, F.pack(payloads, 1))
        # the acquisition's first window is the first frame
        _, acq = R.acquire(sym, P, Rn, word, 1)
        assert acq["sync_window"] == hits["window"][0]
