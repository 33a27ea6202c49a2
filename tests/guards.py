"""Guard bands, poisoned buffers and edge-placed near ties for the device
entry points (tests/test_gpu_guards.py).

The C ABI writes into device pointers its caller owns. Three properties make
it a drop-in library, beyond right values:

  containment   it writes nothing outside its outputs;
  completeness  it writes every element of them;
  isolation     nothing outside the declared input span changes a result.

`guarded` lays an output out as lead | body | tail inside ONE allocation, all
of it poisoned, and hands back the body with a checker: after the run both
guards must still be poison (containment) and no body element may be
(completeness). The poison is a value no legal result has:

  uint8    0xFF        bit 7 is the detectors' "ambiguous" flag (kSymAmbiguous),
                       so a guard byte looks flagged to every rescue scan, and
                       no final symbol carries it;
  float32  0x7FC0DEAD  a NaN's bits, compared as int32; powers are finite, >= 0.

Guards are at least SYM_GUARD bytes (symbols) and F32_GUARD floats (magnitudes,
spectrum) on each side: more than one wave's tile of any kernel (a tile is at
most 64 windows: 64 symbol bytes, 64 x 16 magnitudes, 4 x 513 spectrum
floats). So these tests catch NEAR overruns (one window, one tile, one group
past the end or before the start), not wild pointers, and every stray store
they can see lands inside the guarded allocation. The lead's length modulo 4
sets the body's alignment (an allocation starts 16-byte aligned).

`surrounded` puts the declared input span inside a larger int16 tensor, at
least PCM_SURROUND samples on each side (the lead a multiple of 8 samples:
d_pcm must stay 16-byte aligned), the surroundings all zero or seeded
full-scale noise. An over-read is only ever detected by a result that differs
between surroundings; no buffer is placed at the end of an allocation.

`near_tie_windows` (from tests/test_gpu_decision.py) and `sure_mask` give
windows that the oracle and the host-side error model alone guarantee are
flagged, so that the rescue is reached at the edges where they are placed
(`edge_stream`). A flagged window's symbol and magnitudes are stored by the
rescue, not by the detector's epilogue, so each shape also runs with clean FSK
windows at the same edges: those leave by the epilogue's own stores.

`clear_mask` is sure_mask's counterpart (windows no detector flags) and
`rescue_fixture` the window classes and fixture conditions of the
rescued-magnitude tests (tests/test_gpu_rescue_mags.py); neither needs a
device.
"""
import contextlib
import math
import os

import numpy as np

MAG_TOL = 1e-5                 # of the window's max P (tests/test_gpu_parity.py)
SYM_POISON = 0xFF
F32_POISON = 0x7FC0DEAD
SYM_GUARD = 4096               # bytes per side
F32_GUARD = 16384              # floats per side
PCM_SURROUND = 8192            # samples per side (a multiple of 8)

_INT_VIEW = {"torch.uint8": np.uint8, "torch.int16": np.int16, "torch.float32": np.int32}


@contextlib.contextmanager
def env(**kv):
    """Measurement switches read at demod_create."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def rel_err(mag, P):
    """max_k |mag - P| / max_k P, the largest over the windows."""
    denom = np.maximum(P.max(axis=1), 1e-30)
    return float((np.abs(mag.astype(np.float64) - P).max(axis=1) / denom).max()) if len(P) else 0.0


def guarded(torch, numel, dtype, lead, tail, poison):
    """One flat device allocation lead | body | tail (elements of dtype),
    every element `poison` (float32: its bit pattern). Returns (body, check):
    the body as a contiguous view, and check(written=True), which synchronizes
    and asserts that both guards are still poison and, if `written`, that no
    body element is."""
    flat = torch.empty(lead + numel + tail, dtype=dtype, device="cuda")
    ity = _INT_VIEW[str(dtype)]
    pv = int(poison)
    assert np.iinfo(ity).min <= pv <= np.iinfo(ity).max
    (flat.view(torch.int32) if ity == np.int32 else flat).fill_(pv)
    assert flat.data_ptr() % 16 == 0
    body = flat[lead:lead + numel]
    assert body.is_contiguous() and body.data_ptr() == flat.data_ptr() + lead * flat.element_size()

    def check(written=True):
        torch.cuda.synchronize()
        host = flat.cpu().numpy().view(ity)
        hit = np.flatnonzero(host[:lead] != pv)
        assert hit.size == 0, ("store before the output", (hit[-8:] - lead).tolist())
        hit = np.flatnonzero(host[lead + numel:] != pv)
        assert hit.size == 0, ("store past the output's end", hit[:8].tolist())
        if written:
            b = host[lead:lead + numel]
            miss = np.flatnonzero(b >= 0x80 if ity == np.uint8 else b == pv)
            assert miss.size == 0, ("output elements never written", miss.size, miss[:8].tolist())

    return body, check


def surrounded(torch, x, seed=None, lead=PCM_SURROUND, tail=PCM_SURROUND):
    """The int16 span x inside a larger device tensor: zeros around it, or
    (seed) uniform noise over the full int16 scale +-32767. Returns (body,
    unchanged): the span's view, and a callable asserting that the whole
    tensor still holds what was put there (no kernel writes its input)."""
    assert lead % 8 == 0 and lead >= PCM_SURROUND and tail >= PCM_SURROUND
    x = np.ascontiguousarray(x, np.int16).reshape(-1)
    if seed is None:
        host = np.zeros(lead + x.size + tail, np.int16)
    else:
        host = np.random.default_rng(seed).integers(-32767, 32768, lead + x.size + tail).astype(np.int16)
    host[lead:lead + x.size] = x
    flat = torch.from_numpy(host).cuda()
    body = flat[lead:lead + x.size]
    assert body.data_ptr() % 16 == 0

    def unchanged():
        assert np.array_equal(flat.cpu().numpy(), host), "the input tensor was written to"

    return body, unchanged


def near_tie_windows(freqs, W, seed, n=1024, amp=9000.0):
    """W windows, each two random tones a, b of the plan with random phases;
    b's amplitude is solved (bisection, double precision, before rounding to
    int16) so that the two tones' DFT powers at their own frequencies are in
    ratio P_b / P_a = 1 + eps exactly — including the leakage between them,
    which matters for off-bin plans."""
    rng = np.random.default_rng(seed)
    K = len(freqs)
    t = np.arange(n)
    eps_set = np.array([0.0, 1e-7, 3e-7, 1e-6, 2e-6, 5e-6, 1e-5, 1e-4])
    ab = np.array([rng.choice(K, 2, replace=False) for _ in range(W)])
    eps = eps_set[np.arange(W) % eps_set.size]
    ph = rng.uniform(0, 2 * np.pi, (W, 2))
    w = 2 * np.pi * np.asarray(freqs, np.float64)[ab] / 48000.0          # (W, 2)
    tones = np.cos(w[:, :, None] * t + ph[:, :, None])                  # (W, 2, n)
    E = np.exp(-1j * w[:, :, None] * t)                                  # (W, 2, n)
    c = np.einsum("wjn,wkn->wjk", tones, E)   # c[w, j, k]: tone j's DFT at tone k's frequency

    def ratio(a2):
        Xa = amp * c[:, 0, 0] + a2 * c[:, 1, 0]
        Xb = amp * c[:, 0, 1] + a2 * c[:, 1, 1]
        return np.abs(Xb) ** 2 / np.abs(Xa) ** 2

    lo, hi = np.full(W, 0.5 * amp), np.full(W, 2.0 * amp)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        up = ratio(mid) < 1.0 + eps
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    a2 = 0.5 * (lo + hi)
    v = amp * tones[:, 0] + a2[:, None] * tones[:, 1]
    x = np.clip(np.round(v), -32768, 32767).astype(np.int16)
    return x, ab


def windows_of(x, n, hop, W):
    """The W windows x[w hop : w hop + n] as float64 rows."""
    x = np.asarray(x).reshape(-1)
    v = np.lib.stride_tricks.sliding_window_view(x, n)[::hop][:W]
    assert v.shape[0] == W
    return v.astype(np.float64)


def sure_mask(model, n, xw, ref_P):
    """Windows the detector must flag, by the oracle and the error model alone
    (tests/test_gpu_decision.py `sure`): oracle top-2 margin below half the
    flag threshold tau sqrt(NE P_max), NE the window's energy scale n sum x^2
    (the window folded by 8 for the fold detector: n / 8 sum xf^2). `model` is
    error_model(cfg), xw the windows as float64 rows."""
    W = xw.shape[0]
    if model["energy"] == 1:   # ENERGY_FOLDED
        xf = xw.reshape(W, 8, n // 8).sum(axis=1)
        NE = (n / 8.0) * (xf * xf).sum(axis=1)
    else:
        NE = float(n) * (xw * xw).sum(axis=1)
    Ps = np.sort(np.asarray(ref_P, np.float64), axis=1)
    return (Ps[:, -1] - Ps[:, -2]) < 0.5 * model["tau"] * np.sqrt(NE * Ps[:, -1])


def clear_mask(model, n, xw, ref_P):
    """Windows no detector flags, by the oracle and the error model alone: the
    oracle's top-2 margin above 4 tau sqrt(NE P_max), eight times sure_mask's
    line. With a = sqrt P_1, b = sqrt P_2 of the oracle and d = tau sqrt(NE) /
    4 the two derived bounds' sum, the margin (a - b)(a + b) > 16 d a gives
    a - b > 8 d; the fp32 roots a', b' are within d of them, so the fp32
    margin is at least 6 d (a' + b') >= 6 d a', above the flag line tau
    sqrt(NE_eff) a' = 4 d a' (and above the FFT's, whose Parseval energy is at
    most twice n sum x^2: 5.7 d a')."""
    W = xw.shape[0]
    if model["energy"] == 1:   # ENERGY_FOLDED
        xf = xw.reshape(W, 8, n // 8).sum(axis=1)
        NE = (n / 8.0) * (xf * xf).sum(axis=1)
    else:
        NE = float(n) * (xw * xw).sum(axis=1)
    Ps = np.sort(np.asarray(ref_P, np.float64), axis=1)
    return (Ps[:, -1] - Ps[:, -2]) > 4.0 * model["tau"] * np.sqrt(NE * Ps[:, -1])


def longest_run(mask):
    """Length of the longest run of consecutive True."""
    m = np.concatenate([[0], np.asarray(mask, np.int8), [0]])
    edges = np.flatnonzero(np.diff(m))
    return int((edges[1::2] - edges[::2]).max()) if edges.size else 0


def rescue_fixture(model, x, n, hop, W, ref_P):
    """The window classes of a stream of near-tie runs beside clean FSK
    (error_model.mixed_stream_windows; near_tie_windows with a tie_run) that
    the rescued-magnitude tests stand on, from the oracle's powers and the error
    model alone (no device): `sure` (flagged whatever the fp32 rounding does),
    `clear` (never flagged), `off` (start off a multiple of n: another tile
    position, carried sums). Asserts the fixture conditions: at least 32 sure
    windows, 8 of them off a multiple of n where hop < n, one run of 8 or
    more consecutive sure windows (a dense run of the rescue launch), and 32
    clear windows beside them."""
    xw = windows_of(x, n, hop, W)
    sure = sure_mask(model, n, xw, ref_P)
    clear = clear_mask(model, n, xw, ref_P)
    off = (np.arange(W) * hop) % n != 0
    assert sure.sum() >= 32, int(sure.sum())
    assert hop == n or (sure & off).sum() >= 8, int((sure & off).sum())
    assert clear.sum() >= 32, int(clear.sum())
    assert longest_run(sure) >= 8, longest_run(sure)
    return {"xw": xw, "sure": sure, "clear": clear, "off": off}


def edge_windows(W, T):
    """Where a kernel's hand-written edges are: the batch's first and last
    window, the first and last window of every tile (group) of T windows, and
    both sides of window 512 (the rescue launch's chunk)."""
    w = np.arange(W)
    e = (w == 0) | (w == W - 1) | (w % T == 0) | (w % T == T - 1) | (w == 511) | (w == 512)
    return np.flatnonzero(e)


def edge_stream(pool, edge_idx, n, hop, W, T, fill=None):
    """(W - 1) hop + n samples whose windows at the edges (edge_windows) are
    the pool windows listed in edge_idx (in turn), the rest filled from the
    pool's first `fill` windows (default: all) in a fixed order.
    hop < n: the pool windows are laid end to end, so only windows that start
    on a multiple of n are pool windows (the others are whatever falls out).
    Returns (samples, placed): placed = the edge windows that hold a window of
    edge_idx."""
    P = pool.shape[0] if fill is None else fill
    total = (W - 1) * hop + n
    blocks = -(-total // n)
    src = (np.arange(blocks) * 5 + 1) % P
    period = n // math.gcd(n, hop)          # window w starts a block iff w % period == 0
    placed = [int(w) for w in edge_windows(W, T) if w % period == 0]
    for j, w in enumerate(placed):
        src[w * hop // n] = edge_idx[j % len(edge_idx)]
    x = pool[src].reshape(-1)[:total]
    return np.ascontiguousarray(x), np.array(placed, np.int64)
