"""Where the device entry points write, and what they read (tests/guards.py).

Every other GPU test checks values: symbols exact, magnitudes within 1e-5 of
the double oracle. These check the three properties a library needs that
writes into device pointers its caller owns:

  containment   nothing outside the outputs is written;
  completeness  every element of them is;
  isolation     nothing outside the declared input span changes a result.

Each output sits between poisoned guards (>= 4096 bytes around the symbols,
>= 16384 floats around magnitudes and spectrum: more than one wave's tile of
any kernel, so NEAR overruns are caught, not wild pointers), at every
alignment the ABI accepts; the input span sits inside a larger tensor whose
surroundings are all zero in one run and full-scale noise in the next. Each
run is checked against the double oracle (symbols exact on every window,
magnitudes and spectrum within MAG_TOL of the window's max P) and, bit for
bit, against a clean run of the same handle into fresh exact-size tensors
(the oracle is the truth; the clean run only pins independence of placement).

The inputs reach the decision rescue at the edges: near-tie windows that the
oracle and the error model alone guarantee are flagged (`sure`) stand at the
batch's first and last window, at the first and last window of every tile or
group, and on both sides of window 512 (the rescue launch's chunk); a run
under FSKD_NO_RESCUE=flags shows bit 7 on every such window. A flagged
window's outputs are stored by the rescue, so every shape runs a second time
with clean FSK windows at the same edges (not flagged, by the same run): those
leave by the detector epilogue's own stores. Each case asserts
that it ran the path it names (detector, plan fields, windows per tile,
launches per batch), with and without magnitudes, over window counts 1, 3,
T - 1, T + 1 and 513 for T windows per tile.

No test here can fault the GPU by design: an over-read is detected only as a
result that differs between surroundings, never by placing a buffer next to
unmapped memory, and every guard is wider than any near overrun.
"""
import collections
import functools

import numpy as np
import pytest

import guards as G
from decision import check_decisions
from guards import F32_GUARD, F32_POISON, MAG_TOL, SYM_GUARD, SYM_POISON
from gpu_support import torch  # noqa: F401

pytestmark = pytest.mark.gpu

AUTO, GOERTZEL, FFT, FOLDED, RESIDUE = 0, 1, 2, 3, 4
BIN = 46.875
N = 1024
POOL, POOL_SEED = 512, 5
CLEAN = 64

FSK2 = (1500.0, 3000.0)
FSK8 = tuple(1500.0 + 375.0 * i for i in range(8))
K3 = tuple(BIN * b for b in (40, 64, 120))                  # odd K: the packed pairs' scalar tail
K16 = tuple(BIN * (20 + 7 * i) for i in range(16))          # two candidates per lane
REINSCH2 = (30.0, 23950.0)                                   # |sin w| < 0.1: the Reinsch recurrence
NONINT3 = (1234.5, 2345.6, 4321.0)
FOLD3 = (8 * BIN, 16 * BIN, 504 * BIN)                       # fold, not by 16
FSK8_ODD = tuple(BIN * (32 + 9 * i) for i in range(8))      # every residue class: compile-time classes
ODD5 = FSK8_ODD[:5]                                          # unbalanced: the LDS class file
ODD16 = tuple(BIN * (32 + 9 * i) for i in range(16))


def fold8_at(n):
    """FSK8's shape at window length n: eight tones on multiples of 8 bins."""
    return tuple(48000.0 / n * 8 * (2 + i) for i in range(8))


def odd8_at(n):
    """Eight integer bins over every residue class mod 8 at window length n."""
    return tuple(48000.0 / n * (9 + 5 * i) for i in range(8))


# det: the detector that must run; tile: windows per tile ("direct": 64 / (n /
# 64), "slide": the handle's slide_windows, "fft": groups of 4); sw: the
# handle's slide_windows; launches: kernel launches per batch (the detector's,
# + 1 where the rescue is a launch of its own); info: plan_info fields
Path = collections.namedtuple("Path", "freqs n hop method det tile sw launches info")

PATHS = {
    # plain bank, n = 1024, hop = n (rescue inside the detector kernel)
    "plain_fsk2": Path(FSK2, N, N, GOERTZEL, GOERTZEL, "direct", 0, 1, dict(reinsch=0, slide=0, fold64=1)),
    "plain_k3": Path(K3, N, N, GOERTZEL, GOERTZEL, "direct", 0, 1, dict(reinsch=0, slide=0)),
    "plain_fsk8": Path(FSK8, N, N, GOERTZEL, GOERTZEL, "direct", 0, 1, dict(reinsch=0, slide=0)),
    "plain_k16": Path(K16, N, N, GOERTZEL, GOERTZEL, "direct", 0, 1, dict(reinsch=0, slide=0)),
    "plain_reinsch2": Path(REINSCH2, N, N, AUTO, GOERTZEL, "direct", 0, 1, dict(reinsch=1, slide=0)),
    # fold detector
    "fold_fsk8": Path(FSK8, N, N, FOLDED, FOLDED, "direct", 0, 1, dict(f16=1, slide=0, fold64=1)),
    "fold_fold3": Path(FOLD3, N, N, FOLDED, FOLDED, "direct", 0, 1, dict(f16=0, slide=0, fold64=1)),
    "fold_n256": Path(fold8_at(256), 256, 256, FOLDED, FOLDED, "direct", 0, 2, dict(f16=0, slide=0)),
    "fold_n4096": Path(fold8_at(4096), 4096, 4096, FOLDED, FOLDED, "direct", 0, 2, dict(f16=0, slide=0)),
    # residue detector (its rescue is a launch: pass 0 by the residue fold)
    "residue_fsk8_odd": Path(FSK8_ODD, N, N, RESIDUE, RESIDUE, "direct", 0, 2, dict(dcls=1, fold64=2)),
    "residue_odd5": Path(ODD5, N, N, RESIDUE, RESIDUE, "direct", 0, 2, dict(dcls=0, fold64=2)),
    "residue_odd16": Path(ODD16, N, N, RESIDUE, RESIDUE, "direct", 0, 2, dict(fold64=2)),
    "residue_n256": Path(odd8_at(256), 256, 256, RESIDUE, RESIDUE, "direct", 0, 2, dict(slide=0)),
}
# plain bank, n != 1024: the generic epilogue + rescue_kernel's launch
for _n in (64, 256, 4096):
    for _hop in (_n, _n // 4):
        PATHS[f"plain_nonint3_n{_n}_hop{_hop}"] = Path(NONINT3, _n, _hop, AUTO, GOERTZEL, "direct", 0, 2,
                                                      dict(reinsch=0, slide=0, fold64=0))
# segment-shared windows: SLIDE (48 / H + 1 windows per tile) and fold-slide (4 R)
for _hop, _wt, _wf in ((64, 49, 64), (256, 13, 16), (960, 4, 4)):
    PATHS[f"slide_fsk2_hop{_hop}"] = Path(FSK2, N, _hop, AUTO, GOERTZEL, "slide", _wt, 2, dict(slide=1))
    PATHS[f"fold_slide_fsk8_hop{_hop}"] = Path(FSK8, N, _hop, AUTO, FOLDED, "slide", _wf, 2,
                                              dict(slide=1, f16=1))
# overlapping windows evaluated one by one (hop not a multiple of 64)
for _hop in (200, 8):
    PATHS[f"direct_fsk2_hop{_hop}"] = Path(FSK2, N, _hop, AUTO, GOERTZEL, "direct", 0, 1, dict(slide=0))
    PATHS[f"direct_fold_fsk8_hop{_hop}"] = Path(FSK8, N, _hop, FOLDED, FOLDED, "direct", 0, 1,
                                               dict(slide=0, f16=1))
    PATHS[f"direct_residue_fsk8_odd_hop{_hop}"] = Path(FSK8_ODD, N, _hop, RESIDUE, RESIDUE, "direct", 0, 2,
                                                      dict(slide=0, dcls=1))
# FFT detector, tones only (it rescues in its own kernel)
for _hop in (1024, 256, 200):
    PATHS[f"fft_fsk8_hop{_hop}"] = Path(FSK8, N, _hop, FFT, FFT, "fft", 0, 1, dict())


@functools.lru_cache(maxsize=None)
def pool_windows(freqs, n):
    """The pool of near-tie windows of a plan (shared by the cases on it)."""
    return G.near_tie_windows(freqs, POOL, POOL_SEED, n=n)[0]


def oracle(O, p, x, W):
    if p.det == FFT:
        return O.fft_demod(x, p.freqs, p.n, p.hop)
    return O.goertzel(x, p.freqs, p.n, p.hop, W)


def sure_pool(A, O, p, cfg):
    """(pool, indices of its `sure` windows, the configuration's error model).
    The pool's first POOL windows are near ties, the CLEAN after them clean FSK
    (one tone at 8000, sigma 400)."""
    ties = pool_windows(p.freqs, p.n)
    model = A.error_model(cfg)
    _, P = (O.fft_demod(ties.reshape(-1), p.freqs, p.n) if p.det == FFT else
            O.goertzel(ties.reshape(-1), p.freqs, p.n))
    idx = np.flatnonzero(G.sure_mask(model, p.n, ties.astype(np.float64), P))
    assert idx.size >= 32, idx.size
    clean, _ = O.synth_fsk(p.freqs, p.n, CLEAN, 11, 8000, 400)
    return np.concatenate([ties, clean]), idx, model


def window_counts(T):
    return sorted({1, 3, T - 1, T + 1, 513} - {0})


def launch(d, d_pcm, W, d_sym, d_mag, d_spec):
    if d_spec is not None:
        assert d.batch_spectrum_async(d_pcm, W, d_sym, d_mag, d_spec) == W
    else:
        assert d.batch_async(d_pcm, W, d_sym, d_mag) == W


def fetch(W, K, d_sym, d_mag, d_spec):
    return (d_sym.cpu().numpy(), None if d_mag is None else d_mag.cpu().numpy().reshape(W, K),
            None if d_spec is None else d_spec.cpu().numpy().reshape(W, 513))


def clean_run(d, torch, x, W, K, mags, spec):
    """The same handle into fresh, exact-size, aligned tensors from an
    isolated copy of the input."""
    d_pcm = torch.from_numpy(x.copy()).cuda()
    d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
    d_mag = torch.empty(W * K, dtype=torch.float32, device="cuda") if mags else None
    d_spec = torch.empty(W * 513, dtype=torch.float32, device="cuda") if spec else None
    launch(d, d_pcm, W, d_sym, d_mag, d_spec)
    torch.cuda.synchronize()
    return fetch(W, K, d_sym, d_mag, d_spec)


def guarded_run(d, torch, x, W, K, mags, spec, seed, a_sym, a_mag, a_spec):
    """The input inside its surroundings (zeros, or noise of `seed`), every
    output between poisoned guards, its body a_* elements past a 16-byte
    boundary; the guards and the input are checked after the run."""
    d_pcm, unchanged = G.surrounded(torch, x, seed)
    d_sym, ck_sym = G.guarded(torch, W, torch.uint8, SYM_GUARD + a_sym, SYM_GUARD, SYM_POISON)
    assert d_sym.data_ptr() % 4 == a_sym
    d_mag = d_spec = None
    checks = [ck_sym]
    if mags:
        d_mag, ck = G.guarded(torch, W * K, torch.float32, F32_GUARD + a_mag, F32_GUARD, F32_POISON)
        assert d_mag.data_ptr() % 16 == 4 * a_mag
        checks.append(ck)
    if spec:
        d_spec, ck = G.guarded(torch, W * 513, torch.float32, F32_GUARD + a_spec, F32_GUARD, F32_POISON)
        assert d_spec.data_ptr() % 16 == 4 * a_spec
        checks.append(ck)
    launch(d, d_pcm, W, d_sym, d_mag, d_spec)
    for ck in checks:
        ck()
    unchanged()
    return fetch(W, K, d_sym, d_mag, d_spec)


def check_oracle(got, ref_sym, ref_P, ref_spec):
    sym, mag, spec = got
    bad = np.flatnonzero(sym != ref_sym)
    assert bad.size == 0, ("symbols differ from the oracle", bad[:8].tolist(), sym[bad[:8]], ref_sym[bad[:8]])
    check_decisions(sym, mag, ref_sym, ref_P)
    if mag is not None:
        err = G.rel_err(mag, ref_P)
        assert err <= MAG_TOL, f"magnitude rel err {err:.3e}"
    if spec is not None:
        err = float((np.abs(spec.astype(np.float64) - ref_spec).max(axis=1) / ref_spec.max(axis=1)).max())
        assert err <= MAG_TOL, f"spectrum rel err {err:.3e}"


def check_same_bits(got, clean, what):
    for name, a, b in zip(("symbols", "magnitudes", "spectrum"), got, clean):
        if a is None:
            assert b is None
            continue
        a, b = (a, b) if a.dtype == np.uint8 else (a.view(np.uint32), b.view(np.uint32))
        bad = np.argwhere(a != b)
        assert bad.size == 0, (f"{name} depend on placement ({what})", bad[:8].tolist())


def run_path(A, O, torch, p, mags, spec=False, a_spec=0, counts=None, sym_aligns=None, env=None):
    """One path over its window counts: the path assertions, then per count
    and edge layout (sure near ties at the edges: stored by the rescue; clean
    FSK windows there: stored by the detector's epilogue) the coverage
    assertions, the clean run and the guarded runs in both surroundings (at
    every alignment of sym_aligns, else cycling)."""
    env = env or {}
    K = len(p.freqs)
    cfg = A.make_cfg(n=p.n, hop=p.hop, freqs=p.freqs, method=p.method)
    info = A.plan_info(cfg)
    assert info["method"] == p.det
    for f, v in p.info.items():
        assert info[f] == v, (f, info[f], v)
    pool, sure_idx, model = sure_pool(A, O, p, cfg)
    with G.env(**env):
        d = A.Demodulator(cfg)
    with G.env(FSKD_NO_RESCUE="flags", **env):
        d_flags = A.Demodulator(cfg)
    with d, d_flags:
        assert d.method == p.det and d.slide_windows == p.sw
        assert d.rescue_tau == pytest.approx(model["tau"], rel=1e-12)
        assert (d.rescue_tau64 > 0) == (p.n == 1024)
        T = {"direct": max(1, 64 // (p.n // 64)), "slide": d.slide_windows, "fft": 4}[p.tile]
        assert T >= 1
        run = 0
        for W, layout in [(W, lay) for W in counts or window_counts(T) for lay in ("sure", "clean")]:
            assert d.batch_launches(W, mags) == p.launches
            edge_idx = sure_idx if layout == "sure" else POOL + np.arange(CLEAN)
            x, placed = G.edge_stream(pool, edge_idx, p.n, p.hop, W, T, fill=POOL)
            assert x.size == (W - 1) * p.hop + p.n
            ref_sym, ref_P = oracle(O, p, x, W)
            ref_spec = (np.stack([O.fft_power(x[w * p.hop:w * p.hop + p.n]) for w in range(W)])
                        if spec else None)
            # coverage. The edge windows (hop = n: every one of them; hop < n:
            # those that start a pool window, the first always) are sure, or
            # in the clean layout not flagged; the detector flags every sure
            # window wherever it stands
            sure = G.sure_mask(model, p.n, G.windows_of(x, p.n, p.hop, W), ref_P)
            assert placed.size and placed[0] == 0
            if p.hop == p.n:
                assert np.array_equal(placed, G.edge_windows(W, T))
            flags, _, _ = clean_run(d_flags, torch, x, W, K, False, False)
            assert (flags[sure] & 0x80).all(), np.flatnonzero(sure & ((flags & 0x80) == 0))[:8]
            assert ((flags & 0x7F) < K).all()
            if layout == "sure":
                assert sure[placed].all()
            else:
                assert not (flags[placed] & 0x80).any()
            clean = clean_run(d, torch, x, W, K, mags, spec)
            check_oracle(clean, ref_sym, ref_P, ref_spec)
            for a_sym in sym_aligns or (None,):
                for seed in (None, 1000 + W):
                    a = run % 4 if a_sym is None else a_sym
                    got = guarded_run(d, torch, x, W, K, mags, spec, seed, a, (3 * run + 1) % 4, a_spec)
                    what = (f"W {W}, {layout} edges, {'noise' if seed else 'zeros'} around the input, "
                            f"symbols + {a}")
                    check_oracle(got, ref_sym, ref_P, ref_spec)
                    check_same_bits(got, clean, what)
                    run += 1


@pytest.mark.parametrize("mags", [True, False], ids=["mags", "nomags"])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_detector_paths(A, O, torch, path, mags):
    """Every detector kernel and both rescue forms, W in {1, 3, T - 1, T + 1,
    513}, symbol and magnitude alignments cycling through 0 .. 3."""
    run_path(A, O, torch, PATHS[path], mags)


@pytest.mark.parametrize("mags", [True, False], ids=["mags", "nomags"])
@pytest.mark.parametrize("a_spec", [0, 1, 2, 3])
@pytest.mark.parametrize("hop", [1024, 256])
def test_fft_spectrum_store(A, O, torch, hop, a_spec, mags):
    """demod_batch_spectrum_async at all four float alignments of d_spec (16
    bytes: the linear slab's 16-byte stores with the scalar tail of a partial
    last group; else dword stores). W in {1, 2, 3, 5, 7, 513} leaves 1, 2 and 3
    windows in the last group: every length of the tail."""
    p = Path(FSK8, N, hop, FFT, FFT, "fft", 0, 1, dict())
    run_path(A, O, torch, p, mags, spec=True, a_spec=a_spec, counts=(1, 2, 3, 5, 7, 513))


@pytest.mark.parametrize("mags", [True, False], ids=["mags", "nomags"])
@pytest.mark.parametrize("hop", [1024, 256])
@pytest.mark.parametrize("plan", ["FSK2", "FSK8"])
def test_forced_rescue_launch_symbol_alignments(A, O, torch, plan, hop, mags):
    """FSKD_RESCUE_LAUNCH=1 sends n = 1024 plans through the rescue launch
    (rescue_seg_kernel) at hop = n too; d_sym at all four byte alignments: off
    a 4-byte boundary the launch scans the symbols by bytes."""
    freqs, det = (FSK2, GOERTZEL) if plan == "FSK2" else (FSK8, FOLDED)
    if hop == N:
        p = Path(freqs, N, hop, AUTO, det, "direct", 0, 2, dict(slide=0))
    else:
        p = Path(freqs, N, hop, AUTO, det, "slide", 13 if det == GOERTZEL else 16, 2, dict(slide=1))
    run_path(A, O, torch, p, mags, sym_aligns=(0, 1, 2, 3), env={"FSKD_RESCUE_LAUNCH": "1"})


def test_write_back_bursts(A, O, torch):
    """K = 16 with magnitudes at hop = n, W = 70001: 65 bytes of output per
    window, above the 4 MiB from which a launch writes each XCD's L2 back in
    bursts (demod_api.cpp burst_count: 4 here). One launch; the input is the
    device generator's, inside zero and noise surroundings."""
    n, W, K = N, 70001, 16
    cfg = A.make_cfg(n=n, freqs=K16, method=GOERTZEL)
    assert 4 << 20 < W * (1 + 4 * K) < 10 << 20
    lead = tail = G.PCM_SURROUND
    outs = []
    with A.Demodulator(cfg) as d:
        assert d.method == GOERTZEL and d.batch_launches(W, True) == 1
        for seed in (None, 7):
            if seed is None:
                flat = torch.zeros(lead + W * n + tail, dtype=torch.int16, device="cuda")
            else:
                g = torch.Generator(device="cuda").manual_seed(seed)
                flat = torch.randint(-32767, 32768, (lead + W * n + tail,), dtype=torch.int16, device="cuda",
                                     generator=g)
            around = torch.cat([flat[:lead], flat[lead + W * n:]]).clone()
            d_pcm = flat[lead:lead + W * n]
            d_true, ck_true = G.guarded(torch, W, torch.uint8, SYM_GUARD, SYM_GUARD, SYM_POISON)
            A.synth_fsk(cfg, 99, W, 8000, 400, d_pcm, d_true)
            ck_true()
            d_sym, ck_sym = G.guarded(torch, W, torch.uint8, SYM_GUARD + 3, SYM_GUARD, SYM_POISON)
            d_mag, ck_mag = G.guarded(torch, W * K, torch.float32, F32_GUARD + 1, F32_GUARD, F32_POISON)
            assert d.batch_async(d_pcm, W, d_sym, d_mag) == W
            ck_sym()
            ck_mag()
            assert torch.equal(torch.cat([flat[:lead], flat[lead + W * n:]]), around)
            outs.append((d_pcm.cpu().numpy(), d_true.cpu().numpy(),
                         fetch(W, K, d_sym, d_mag, None)))
        (x, truth, got0), (x1, truth1, got1) = outs
        assert np.array_equal(x, x1) and np.array_equal(truth, truth1)
        clean = clean_run(d, torch, x, W, K, True, False)
    ref_sym, ref_P = O.goertzel(x, K16, n, n, W, threads=16)
    assert np.array_equal(ref_sym, truth)
    for got, what in ((got0, "zeros"), (got1, "noise")):
        check_oracle(got, ref_sym, ref_P, None)
        check_same_bits(got, clean, what)


@pytest.mark.parametrize("bits", [1, 3, 4])
@pytest.mark.parametrize("n_streams", [1, 3])
def test_frame_streams_guarded(A, torch, n_streams, bits):
    """demod_frame_streams_async around the frame boundary (n = 1, per - 1,
    per, per + 1 symbols for per symbols per full frame): the output between
    guards, the symbols inside surroundings of the same poison; bytes equal to
    the host codec. A frame byte may take any value, so each shape runs with
    poison 0xFF and 0x00: a byte the kernel leaves out differs in one of them."""
    per = A.DEMOD_MAX_FRAME_PAYLOAD * 8 // bits
    rng = np.random.default_rng(100 * n_streams + bits)
    run = 0
    for n in (1, per - 1, per, per + 1):
        sym = rng.integers(0, 256, (n_streams, n), dtype=np.uint8)
        stride = A.frame_symbols_size(n, bits)
        ref = b"".join(A.frame_symbols(sym[s], bits) for s in range(n_streams))
        assert len(ref) == n_streams * stride
        for poison in (0xFF, 0x00):
            d_in, ck_in = G.guarded(torch, n_streams * n, torch.uint8, SYM_GUARD + (run + 1) % 4, SYM_GUARD,
                                    poison)
            d_in.copy_(torch.from_numpy(sym.reshape(-1)))
            d_out, ck_out = G.guarded(torch, n_streams * stride, torch.uint8, SYM_GUARD + run % 4,
                                      SYM_GUARD, poison)
            assert A.frame_streams_async(d_in, n_streams, n, bits, d_out) == stride
            ck_out(written=False)
            ck_in(written=False)
            assert d_out.cpu().numpy().tobytes() == ref, (n, poison)
            assert np.array_equal(d_in.cpu().numpy(), sym.reshape(-1))
            run += 1


def test_synth_fsk_guarded(A, O, torch):
    """The device generator at n = 64, W = 3: PCM and symbols between guards,
    equal to the CPU generator. Any int16 is a legal sample, so the PCM's
    completeness is its equality with the CPU generator's (which never
    produces the poison -32768 at this level)."""
    n, W, freqs = 64, 3, (700.0, 1234.5, 9000.0)
    cfg = A.make_cfg(n=n, freqs=freqs)
    pcm, sym = O.synth_fsk(freqs, n, W, 77, 8000, 400)
    assert (pcm != -32768).all()
    for a in range(4):
        d_pcm, ck_pcm = G.guarded(torch, W * n, torch.int16, G.PCM_SURROUND + 8 * a, G.PCM_SURROUND, -32768)
        d_sym, ck_sym = G.guarded(torch, W, torch.uint8, SYM_GUARD + a, SYM_GUARD, SYM_POISON)
        A.synth_fsk(cfg, 77, W, 8000, 400, d_pcm, d_sym)
        ck_pcm(written=False)
        ck_sym()
        assert np.array_equal(d_pcm.cpu().numpy().reshape(W, n), pcm)
        assert np.array_equal(d_sym.cpu().numpy(), sym)
        d_pcm, ck_pcm = G.guarded(torch, W * n, torch.int16, G.PCM_SURROUND, G.PCM_SURROUND, -32768)
        A.synth_fsk(cfg, 77, W, 8000, 400, d_pcm, None)
        ck_pcm(written=False)
        assert np.array_equal(d_pcm.cpu().numpy().reshape(W, n), pcm)


@pytest.mark.parametrize("method", [AUTO, FFT])
def test_refused_batch_writes_nothing(A, torch, method):
    """A d_pcm 2 bytes off 16-byte alignment is refused with DEMOD_BAD_ARG by
    every batch entry point, and the poisoned outputs stay untouched."""
    W, K = 5, 2
    flat = torch.zeros(G.PCM_SURROUND + 1 + W * N, dtype=torch.int16, device="cuda")
    d_pcm = flat[G.PCM_SURROUND + 1:]
    assert d_pcm.data_ptr() % 16 == 2
    d_sym, ck_sym = G.guarded(torch, W, torch.uint8, SYM_GUARD, SYM_GUARD, SYM_POISON)
    d_mag, ck_mag = G.guarded(torch, W * K, torch.float32, F32_GUARD, F32_GUARD, F32_POISON)
    d_spec, ck_spec = G.guarded(torch, W * 513, torch.float32, F32_GUARD, F32_GUARD, F32_POISON)
    with A.Demodulator(freqs=FSK2, method=method) as d:
        calls = [lambda: d.batch_async(d_pcm, W, d_sym, d_mag), lambda: d.batch_device(d_pcm, W, d_sym, d_mag)]
        if method == FFT:
            calls.append(lambda: d.batch_spectrum_async(d_pcm, W, d_sym, d_mag, d_spec))
        for call in calls:
            with pytest.raises(A.DemodError) as e:
                call()
            assert e.value.code == A.DEMOD_BAD_ARG
    for t, ck, pv in ((d_sym, ck_sym, SYM_POISON), (d_mag, ck_mag, F32_POISON), (d_spec, ck_spec, F32_POISON)):
        ck(written=False)
        body = t.cpu().numpy()
        assert ((body if body.dtype == np.uint8 else body.view(np.int32)) == pv).all()


@pytest.mark.parametrize("case", ["fsk2", "fsk8", "fft_fsk2_hop256"])
def test_past_4gib(A, O, torch, case):
    """Batches whose input byte offsets cross 2^31 and 2^32 (2^21 + 5 windows
    of 1024 samples, just over 4 GiB, from the device generator; the FFT case
    slides over the same samples at hop 256), outputs guarded at the tail.
    Every window aligned to n decodes to the transmitted symbol, and a
    4096-window sample (the last 16 windows and the 16 around each of the two
    byte offsets included) equals the oracle, magnitudes inside MAG_TOL."""
    n, src = N, (1 << 21) + 5
    freqs, method, det, hop = {"fsk2": (FSK2, AUTO, GOERTZEL, n), "fsk8": (FSK8, AUTO, FOLDED, n),
                               "fft_fsk2_hop256": (FSK2, FFT, FFT, 256)}[case]
    K = len(freqs)
    d_pcm = torch.empty(src * n, dtype=torch.int16, device="cuda")
    d_true = torch.empty(src, dtype=torch.uint8, device="cuda")
    A.synth_fsk(A.make_cfg(n=n, freqs=freqs), A.BENCH_SEED, src, 8000, 400, d_pcm, d_true)
    W = (src * n - n) // hop + 1
    assert ((W - 1) * hop + n) * 2 > 1 << 32
    d_sym, ck_sym = G.guarded(torch, W, torch.uint8, 0, SYM_GUARD, SYM_POISON)
    d_mag, ck_mag = G.guarded(torch, W * K, torch.float32, 0, F32_GUARD, F32_POISON)
    with A.Demodulator(n=n, hop=hop, freqs=freqs, method=method) as d:
        assert d.method == det
        assert d.batch_device(d_pcm, W, d_sym, d_mag) == W
    ck_sym()
    ck_mag()
    assert torch.equal(d_sym[::n // hop], d_true)
    near = [np.arange(W - 16, W)]
    for off in (1 << 31, 1 << 32):
        w0 = off // (2 * hop)          # the window that starts at that byte
        near.append(np.arange(w0 - 8, w0 + 8))
    near = np.concatenate(near)
    near = near[(near >= 0) & (near < W)]
    rest = np.setdiff1d(np.arange(W), near)
    idx = np.sort(np.concatenate([near, np.random.default_rng(3).choice(rest, 4096 - near.size,
                                                                        replace=False)]))
    ti = torch.from_numpy(idx).cuda()
    pos = ti[:, None] * hop + torch.arange(n, device="cuda")[None, :]
    pcm = d_pcm[pos].cpu().numpy()
    ref_sym, ref_P = (O.fft_demod if det == FFT else O.goertzel)(pcm, freqs, n)
    assert np.array_equal(d_sym[ti].cpu().numpy(), ref_sym)
    assert G.rel_err(d_mag.view(W, K)[ti].cpu().numpy(), ref_P) <= MAG_TOL
    del d_pcm
