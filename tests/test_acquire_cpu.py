"""Acquisition without a GPU: the ABI (exports, struct layout, workspace size)
and the reference of tests/acquire_ref.py on the oracle's sliding-window
powers, cases A-D of DESIGN.md §4.9."""
import ctypes

import numpy as np
import pytest

import acquire_ref as R


def test_exports_and_result_struct(A):
    lib = A.load_library()
    for name in ("demod_acquire_workspace_size", "demod_acquire_async", "demod_acquire"):
        assert hasattr(lib, name), name
        assert name in A.header_exports()
    T = A.DemodAcquireResult
    assert ctypes.sizeof(T) == R.RESULT_DTYPE.itemsize and [f for f, _ in T._fields_] == list(R.RESULT_DTYPE.names)
    for f in R.RESULT_DTYPE.names:                                  # every field where the tests' one dtype has it
        at, size = R.RESULT_DTYPE.fields[f][1], R.RESULT_DTYPE[f].itemsize
        assert (getattr(T, f).offset, getattr(T, f).size) == (at, size), f
    assert A.DEMOD_MAX_PHASES == 64 and A.DEMOD_MAX_SYNC == 64
    hdr = open(A.HEADER_PATH).read()
    assert "#define DEMOD_ACQUIRE_TILE %d" % A.ACQUIRE_TILE in hdr
    assert A.ACQUIRE_TILE % 64 == 0


def test_workspace_size(A):
    sizes = {}
    for n, hop in [(1024, 1024), (1024, 512), (1024, 256), (1024, 64), (1024, 16), (256, 64),
                   (4096, 64), (512, 8), (64, 8)]:
        s = A.acquire_workspace_size(A.make_cfg(n=n, hop=hop))
        assert s > 0 and s % 8 == 0
        sizes[n // hop] = s
    assert sizes[64] >= sizes[16] >= sizes[4] >= sizes[1]
    # hop does not divide n; more than 64 phases; an invalid configuration
    for n, hop in [(1024, 384), (1024, 8), (4096, 8), (4096, 32), (1000, 250)]:
        cfg = A.make_cfg(n=n, hop=hop)
        assert A.load_library().demod_acquire_workspace_size(ctypes.byref(cfg)) == 0
        with pytest.raises(A.DemodError) as e:
            A.acquire_workspace_size(cfg)
        assert e.value.code == A.DEMOD_BAD_ARG
    assert A.load_library().demod_acquire_workspace_size(None) == 0


def test_async_refuses_null_handle(A):
    lib = A.load_library()
    res = A.DemodAcquireResult()
    assert lib.demod_acquire_async(None, None, None, 4, None, 0, 0, None, 0, None, None,
                                   None) == A.DEMOD_BAD_ARG
    assert lib.demod_acquire(None, None, 4, None, 0, 0, None, 0, ctypes.byref(res)) == A.DEMOD_BAD_ARG


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_reference_on_the_oracle(O, name):
    """The per-phase sum of the decided tone's power over the oracle's double
    sliding-window powers peaks at the true phase; with the sync word
    truth[5:29] the symbols after it are truth[29:]."""
    freqs, n, hop, _, _, m_on, m_off = R.CASES[name]
    Rn = n // hop
    for tau, want in R.case_taus(n, hop):
        x, truth = R.case_stream(O, name, tau)
        sym, P = O.goertzel(x, freqs, n, hop)
        word = truth[5:29]
        out, res = R.acquire(sym, P, Rn, word, 0)
        m = R.margin(res["metric"])
        print(f"case {name} tau {tau}: W {len(sym)} phase {res['phase']} margin {m:.4f} "
              f"sync_window {res['sync_window']} n_out {res['n_out']}")
        assert res["phase"] == want == (tau + hop // 2) // hop
        # the table's margins (another noise draw: within 15 %), all >> 4e-5
        table = m_on if tau % hop == 0 else m_off
        assert abs(m - table) <= 0.15 * table and m > 4e-5
        stream = sym[res["phase"]::Rn]
        hits = [i for i in range(len(stream) - 23) if (stream[i:i + 24] == word).all()]
        assert hits == [5], hits
        assert res["sync_window"] == res["phase"] + 5 * Rn and res["sync_errors"] == 0
        assert res["first_window"] == res["phase"] + 29 * Rn
        assert res["n_out"] == len(out) > 0
        assert np.array_equal(out, truth[29:29 + len(out)])
        assert len(truth) - 29 - len(out) <= 1   # all but a cut last symbol


def test_reference_definitions():
    """Hand-made cases of the definitions: ties, bytes >= K, the tail, the
    last legal start, max_errors, cap."""
    K, Rn = 2, 2
    sym = np.array([0, 1, 1, 0, 0x80, 1, 0xFF, 0, 1], np.uint8)      # W = 9: J = 4, tail w = 8
    P = np.arange(18, dtype=np.float64).reshape(9, 2) + 1.0
    M, J = R.phase_metric(sym, P, Rn)
    assert J == 4 and M[0] == P[0, 0] + P[2, 1] and M[1] == P[1, 1] + P[3, 0] + P[5, 1] + P[7, 0]
    _, res = R.acquire(sym, np.ones((9, K)), Rn)                      # M = [2, 4]
    assert res["phase"] == 1 and res["first_window"] == 1 and res["n_out"] == 4
    _, res = R.acquire(np.zeros(8, np.uint8), np.ones((8, K)), Rn)    # a tie: the lowest
    assert res["phase"] == 0 and res["sync_window"] == -1
    sym = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8)               # phase 0 stream: 1 1 0 1
    P = np.ones((8, K))
    P[::2] = 2.0
    out, res = R.acquire(sym, P, Rn, [1, 0, 1], 0)                    # phase 1 has no say
    assert res["phase"] == 0 and res["sync_window"] == 2 and res["n_out"] == 0 and out.size == 0
    assert res["first_window"] == 8
    out, res = R.acquire(sym, P, Rn, [1, 0], 0, cap=1)
    assert res["sync_window"] == 2 and res["first_window"] == 6 and res["n_out"] == 1
    assert out.tolist() == [1]
    out, res = R.acquire(sym, P, Rn, [0, 0], 1)                       # one error allowed: w = 2
    assert res["sync_window"] == 2 and res["sync_errors"] == 1
    out, res = R.acquire(sym, P, Rn, [0, 0], 0)
    assert res["sync_window"] == -1 and res["n_out"] == 0 and res["first_window"] == 8
    assert R.sync_errors(sym, Rn, [1, 0, 1], 2) == 0 and R.sync_errors(sym, Rn, [1, 0, 1], 3) == 1
    assert R.sync_errors(sym, Rn, [1, 0, 1], 4) is None
