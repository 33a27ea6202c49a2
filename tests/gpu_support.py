"""What the GPU tests share: the torch and handle fixtures, whole-output
comparison, a hand-built frames result, and the helpers that were the same
function in several test files. A plain module: a test file imports what it
uses by name (pytest finds a fixture in the namespace it was imported into;
a module-scoped one is made once per requesting module).

pytest does not rewrite the asserts of this module, so each carries its message.
"""
import inspect

import numpy as np
import pytest

import frames_ref as F
import guards as G

LEAD = 4096          # guard bytes per side (a multiple of 8: aligned outputs stay aligned)
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU visible")
    return t


def handle_fixture(make):
    """A module-scoped fixture `handle`: handle(*key) is make(A, *key), made once
    per key (make's defaults filled in) and closed when the module ends."""
    sig = inspect.signature(make)

    @pytest.fixture(scope="module")
    def handle(A, torch):
        made = {}

        def get(*key):
            bound = sig.bind(A, *key)
            bound.apply_defaults()
            key = bound.args[1:]
            if key not in made:
                made[key] = make(A, *key)
            return made[key]
        yield get
        for d in made.values():
            d.close()
    return handle


def tones_375(K):
    return tuple(1500.0 + 375.0 * i for i in range(K))


def phased(A, shape_of_r, Rn, freqs):
    """A Demodulator with R = n / hop phases, (n, hop) = shape_of_r[R]."""
    n, hop = shape_of_r[Rn]
    d = A.Demodulator(n=n, hop=hop, freqs=freqs)
    assert d.n // d.hop == Rn, (d.n, d.hop, Rn)
    return d


def same(got, want, what="", names=None):
    """Whole arrays equal: a dict of arrays against a dict (by key), a tuple of
    arrays against a tuple (named by `names`), or one array against one,
    flattened (there the first got / want values are shown too)."""
    if isinstance(got, dict):
        names, got, want = list(got), list(got.values()), [want[k] for k in got]
    if names is None:
        got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, bad.size, bad[:6].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())
        return
    for name, g, w in zip(names, got, want):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist())


def results_bytes(n_written):
    """[G] demod_frames_result_t with n_hits = n_written = the given counts, the rest 0."""
    res = np.zeros(len(n_written), F.RESULT_DTYPE)
    res["n_hits"] = res["n_written"] = np.array([int(n) for n in n_written], "<u8")
    return res.view(np.uint8).reshape(len(n_written), F.RESULT_DTYPE.itemsize)


def guarded(torch, numel, lead, poison):
    """guards.guarded for a uint8 output; (None, a check of nothing) for an empty one."""
    if numel == 0:
        return None, lambda written: None
    return G.guarded(torch, numel, torch.uint8, lead, LEAD, poison)


def tables(torch, first, count):
    """The uint64 / uint32 tables as the int64 / int32 tensors that carry them."""
    f = np.ascontiguousarray(first, np.uint64).view(np.int64)
    c = np.ascontiguousarray(count, np.uint32).view(np.int32)
    return torch.from_numpy(f.copy()).cuda(), torch.from_numpy(c.copy()).cuda()


def parse_acquire(A, raw):
    return A.acquire_result_dict(A.DemodAcquireResult.from_buffer_copy(bytes(raw)))


def parse_frames(A, raw):
    return A.frames_result_dict(A.DemodFramesResult.from_buffer_copy(bytes(raw)))


# ---- acquisition (test_gpu_acquire.py, test_gpu_acquire_segments.py) ---------------------

ACQUIRE_INT_FIELDS = ("phases", "phase", "per_phase", "sync_window", "sync_errors", "reserved",
                      "first_window", "n_out")


def check_acquire(res, out, ref_out, ref, cap, metric=True):
    """One acquisition's result dict and output bytes against the reference's:
    the integer fields equal, the metric within J 2^-52 M_ref, bytes past
    n_written untouched."""
    for f in ACQUIRE_INT_FIELDS:
        assert res[f] == ref[f], (f, res[f], ref[f])
    assert res["n_written"] == min(ref["n_out"], cap), ("n_written", res["n_written"], ref["n_out"], cap)
    nw = res["n_written"]
    assert np.array_equal(out[:nw], ref_out[:nw]), ("output bytes", out[:nw], ref_out[:nw])
    assert (out[nw:] == 0xFF).all(), "bytes past n_written were written"
    if metric:
        M, Mr = res["metric"], ref["metric"]
        assert M.shape == Mr.shape, (M.shape, Mr.shape)
        assert (np.abs(M - Mr) <= ref["per_phase"] * EPS * Mr).all(), (M, Mr)


# ---- the frame scan (test_gpu_frames.py, test_gpu_frames_segments.py) ----------------------

def frames_result_bytes(A, ref):
    r = A.DemodFramesResult()
    for i, m in enumerate(ref["metric"]):
        r.metric[i] = float(m)
    for f in ("phases", "phase", "per_phase", "n_hits", "n_written", "tail_window", "tail_errors",
              "reserved"):
        setattr(r, f, int(ref[f]))
    return bytes(r)


def check_frames(A, out, ref, max_frames, poison=0xFF):
    """One scan (or one segment's): result bytes, hits, payload rows and packed
    rows equal the reference's; rows past n_written still hold the poison."""
    r_hits, r_pay, r_pak, r_res = ref
    r_res = dict(r_res, n_written=min(r_res["n_hits"], max_frames))
    nw = r_res["n_written"]
    assert out["raw"] == frames_result_bytes(A, r_res), (out["res"], r_res)
    assert out["hits"][:nw].tobytes() == r_hits[:nw].tobytes(), ("hits", out["hits"][:nw], r_hits[:nw])
    assert (out["hits"][nw:].view(np.uint8) == poison).all(), "hit rows past n_written were written"
    for name, got, want in (("payload", out["payload"], r_pay), ("packed", out["packed"], r_pak)):
        if got is not None:
            assert np.array_equal(got[:nw], want[:nw]), (name, got[:nw], want[:nw])
            assert (got[nw:] == poison).all(), "rows past n_written were written"
