"""GPU parity: the HIP path (through the C ABI) against the CPU oracle.

Bar (BASELINE.json north_star): symbol indices bit-exact; tone magnitudes
within 1e-5 relative, measured as max_k |P_gpu - P_ref| / max_k P_ref per
window, P_ref from the double-precision oracle.
"""
import numpy as np
import pytest

from decision import check_decisions
from gpu_support import torch  # noqa: F401

pytestmark = pytest.mark.gpu

MAG_TOL = 1e-5  # relative to the window's max_k P_ref (north_star)


def rel_err(mag, P):
    denom = np.maximum(P.max(axis=1), 1e-30)
    return float((np.abs(mag.astype(np.float64) - P).max(axis=1) / denom).max()) if len(P) else 0.0


def run_case(A, O, freqs, n=1024, W=257, hop=None, seed=1, amplitude=8000, sigma=400,
             method=0, check_truth=True):
    pcm, truth = O.synth_fsk(freqs, n, W, seed, amplitude, sigma)
    flat = pcm.reshape(-1)
    hop = n if hop is None else hop
    Wh = (flat.size - n) // hop + 1
    with A.Demodulator(n=n, hop=hop, freqs=freqs, method=method) as d:
        if method:
            assert d.method == method
        sym, mag = d.batch(flat, n_windows=Wh, mags=True)
    ref_sym, ref_P = O.goertzel(flat, freqs, n, hop, Wh)
    assert sym.shape == ref_sym.shape
    check_decisions(sym, mag, ref_sym, ref_P)
    mism = int((sym != ref_sym).sum())
    err = rel_err(mag, ref_P)
    assert mism == 0, f"{mism} symbol mismatches"
    assert err <= MAG_TOL, f"magnitude rel err {err:.3e}"
    if hop == n and check_truth:
        # clean windows: the decision must also recover the transmitted symbol
        assert (sym == truth).mean() > 0.999 if sigma <= 400 else True
    return err


GOERTZEL, FFT, FOLDED, RESIDUE = 1, 2, 3, 4
# 8-FSK on integer bins 32 + 9 i (46.875 Hz spacing): bins 32..95 hit every
# residue class mod 8, so only the residue detector folds this plan
FSK8_ODD = tuple(46.875 * (32 + 9 * i) for i in range(8))


@pytest.mark.parametrize("method", [GOERTZEL, FOLDED, RESIDUE])
@pytest.mark.parametrize("W", [1, 2, 3, 4, 5, 63, 1000, 4097])
def test_fsk2_window_counts(A, O, torch, W, method):
    run_case(A, O, A.FSK2_FREQS, W=W, seed=W, method=method)


@pytest.mark.parametrize("method", [GOERTZEL, FOLDED, RESIDUE])
def test_fsk8(A, O, torch, method):
    run_case(A, O, A.FSK8_FREQS, W=3001, seed=8, method=method)


@pytest.mark.parametrize("method", [GOERTZEL, RESIDUE])
def test_fsk8_every_residue_class(A, O, torch, method):
    run_case(A, O, FSK8_ODD, W=3001, seed=88, method=method)


@pytest.mark.parametrize("k", list(range(1, 17)))
def test_residue_tone_counts_integer_bins(A, O, torch, k):
    # random distinct integer bins >= 3 apart, every residue class mod 8 in play
    rng = np.random.default_rng(500 + k)
    while True:
        b = np.sort(rng.choice(np.arange(8, 500), k, replace=False))
        if k == 1 or np.diff(b).min() >= 3:
            break
    freqs = tuple(float(x) * 46.875 for x in rng.permutation(b))
    run_case(A, O, freqs, W=333, seed=k, method=RESIDUE)


@pytest.mark.parametrize("bins,hop", [
    ([32 + 9 * i for i in range(8)][::-1], 1024),          # every residue once, reversed
    ([95 - 9 * i for i in (3, 0, 6, 1, 7, 2, 5, 4)], 1024),  # same set, scrambled
    ([8, 16, 9, 17, 11, 19, 10, 18], 1024),                 # residues 0,0,1,1,3,3,2,2
    ([40, 44, 33, 39, 35, 37, 42, 46], 256),                # 0,4,1,7,3,5,2,6 (pairs share a class)
    ([32 + 9 * i for i in range(16)], 1024),                # K = 16: every class 4 times
    ([200 - 9 * i for i in range(16)], 512),
    # even bins (round 2, DC modes 2-4: only the classes read are formed)
    ([32 + 2 * i for i in range(8)], 1024),                 # spacing 2: classes 0 | 3, 4 + 4
    ([74 - 6 * i for i in range(8)], 1024),                 # spacing 6, descending
    ([34 + 2 * i for i in range(16)][::-1], 512),           # K = 16, 8 + 8
    ([36 + 4 * i for i in (5, 2, 7, 0, 3, 6, 1, 4)], 1024), # spacing 4 from 36: class 0 only
    ([20 + 24 * i for i in range(8)], 256),                 # residues 4, 0, 4, ...: class 0 only
    ([34 + 4 * i for i in range(8)], 1024),                 # residues 2 / 6: class 3 only
    ([2 + 8 * i for i in range(16)][::-1], 1024),           # K = 16, class 3 only
])
def test_residue_compile_time_classes(A, O, torch, bins, hop):
    """Plans with a compile-time class pattern (n = 1024, K = 8 or 16): K / 4
    tones in every residue class, or even bins split K / 2 + K / 2 over
    classes 0 and 3, or all in class 0 or all in class 3. The residue
    detector permutes the tones so each kernel slot reads a fixed class from
    registers (residue.hip DC) and the window_sum epilogue maps magnitudes,
    the tie rule and the symbol back to the caller's tone order."""
    freqs = tuple(b * 46.875 for b in bins)
    run_case(A, O, freqs, W=700, hop=hop, seed=sum(bins), method=RESIDUE)
    # exact ties (all-zero window) still go to the caller's lowest tone index
    x = np.zeros((3, 1024), np.int16)
    x[1] = np.round(8000 * np.cos(2 * np.pi * bins[5] * np.arange(1024) / 1024))
    with A.Demodulator(freqs=freqs, method=RESIDUE) as d:
        sym, mag = d.batch(x, mags=True)
    assert sym[0] == 0 and sym[2] == 0 and (mag[0] == 0).all()
    assert sym[1] == 5 and int(np.argmax(mag[1])) == 5


@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024, 2048, 4096])
@pytest.mark.parametrize("hop_div", [1, 4])
def test_residue_all_lengths(A, O, torch, n, hop_div):
    # integer bins 3, 4, 5, ... for this n (bin spacing fs/n): every class
    k_max = min(8, n // 2 - 4)
    freqs = tuple((3 + 5 * i) * 48000.0 / n for i in range(k_max) if 3 + 5 * i < n // 2)
    run_case(A, O, freqs, n=n, W=120, hop=n // hop_div, seed=n + hop_div, method=RESIDUE)


def test_residue_rejects_noninteger_bins(A, torch):
    with pytest.raises(A.DemodError) as e:
        A.Demodulator(freqs=(1500.0, 1510.0, 3000.0), method=RESIDUE)
    assert e.value.code == A.DEMOD_BAD_ARG


def test_auto_method_selection(A, torch):
    with A.Demodulator(freqs=A.FSK8_FREQS) as d:
        assert d.method == FOLDED            # K >= 3 on multiples of 8 bins
    with A.Demodulator(freqs=A.FSK2_FREQS) as d:
        assert d.method == GOERTZEL          # plain tone bank already HBM-bound
    with A.Demodulator(freqs=(1500.0, 1546.875, 3000.0)) as d:
        assert d.method == GOERTZEL          # bin 33, K = 3: plain bank as fast
    with A.Demodulator(freqs=FSK8_ODD[:5]) as d:
        assert d.method == RESIDUE           # integer bins, not multiples of 8, K >= 5
    with A.Demodulator(freqs=FSK8_ODD) as d:
        assert d.method == RESIDUE
    with A.Demodulator(freqs=(1500.0, 1510.0, 3000.0)) as d:
        assert d.method == GOERTZEL          # 1510 Hz: not an integer bin
    with A.Demodulator(freqs=(1500.0, 1546.875)) as d:
        assert d.method == GOERTZEL          # K = 2: plain bank is HBM-bound


@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024, 2048, 4096])
@pytest.mark.parametrize("hop_div", [1, 4])
def test_folded_all_lengths(A, O, torch, n, hop_div):
    # tones on multiples of 8 bins for this n (bin spacing fs/n)
    step = 8 * 48000.0 / n
    k_max = min(8, int((n // 2) // 8) - 1)  # stay below Nyquist
    freqs = tuple(step * (i + 1) for i in range(k_max))
    run_case(A, O, freqs, n=n, W=120, hop=n // hop_div, seed=n + hop_div, method=FOLDED)


@pytest.mark.parametrize("n", [64, 128, 256, 512, 2048, 4096])
def test_window_lengths(A, O, torch, n):
    run_case(A, O, A.FSK2_FREQS, n=n, W=300, seed=n)
    run_case(A, O, A.FSK8_FREQS, n=n, W=200, seed=n + 1)


@pytest.mark.parametrize("k", list(range(1, 17)))
def test_tone_counts_noninteger_bins(A, O, torch, k):
    # random non-integer-bin tones, >= 3 bins (140.6 Hz) apart
    rng = np.random.default_rng(100 + k)
    while True:
        f = np.sort(rng.uniform(300.0, 20000.0, k))
        if k == 1 or np.diff(f).min() > 140.625:
            break
    run_case(A, O, tuple(rng.permutation(f)), W=333, seed=k)


@pytest.mark.parametrize("n", [64, 256, 1024, 4096])
@pytest.mark.parametrize("method", [GOERTZEL, RESIDUE])
def test_edge_frequencies(A, O, torch, n, method):
    """Tones near 0 and fs/2, where the fp32 coefficient 2cos(w) cannot resolve
    w (fp32 emulation of the 2cos(w) chain: 4-8e-5 of P at |sin w| ~ 0.01). The
    plain bank switches such plans to the Reinsch-modified recurrence
    (goertzel.hip RS); the residue kernel's 8-sample chains stay within the bar."""
    h = n // 2
    bins = [1, 2, 3, h - 3, h - 1] if n > 64 else [1, 2, 3, 29, 31]
    if method == GOERTZEL:
        bins = bins + [0.5, h - 0.5, h / 2 + 0.3]
    freqs = tuple(b * 48000.0 / n for b in bins)
    for amp, sigma in ((300, 0), (8000, 400), (30000, 100)):
        # tones half a bin apart (0.5 / 1, h - 1 / h - 0.5) are not separable:
        # parity with the oracle is the bar here, not symbol recovery
        run_case(A, O, freqs, n=n, W=200, seed=n + amp, amplitude=amp, sigma=sigma,
                 method=method, check_truth=False)
    run_case(A, O, freqs, n=n, W=60, hop=max(8, n // 4), seed=n + 1, method=method)


@pytest.mark.parametrize("method", [GOERTZEL, FFT])
def test_dc_and_nyquist_tones(A, O, torch, method):
    """Tones exactly at 0 Hz and fs/2 (the ABI accepts [0, fs/2]): lambda = 0
    with sgn = +1 / -1 in the Reinsch form, bins 0 and 512 in the FFT's
    pair-slot layout."""
    freqs = (0.0, 1500.0, 24000.0, 3000.0)
    pcm, _ = O.synth_fsk(freqs, 1024, 300, 42, 8000, 400)
    with A.Demodulator(freqs=freqs, method=method) as d:
        sym, mag = d.batch(pcm, mags=True)
    ref_sym, ref_P = (O.fft_demod if method == FFT else O.goertzel)(pcm, freqs, 1024)
    assert (sym == ref_sym).all()
    assert rel_err(mag, ref_P) <= MAG_TOL


@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_edge_frequencies_folded(A, O, torch, n):
    h = n // 2
    freqs = tuple(b * 48000.0 / n for b in (8, 16, h - 16, h - 8))
    for amp, sigma in ((300, 0), (8000, 400)):
        run_case(A, O, freqs, n=n, W=200, seed=n + amp, amplitude=amp, sigma=sigma,
                 method=FOLDED)


@pytest.mark.parametrize("hop", [8, 256, 512, 1000])
def test_sliding_hop(A, O, torch, hop):
    run_case(A, O, A.FSK2_FREQS, W=40, hop=hop, seed=hop)


@pytest.mark.parametrize("method", [GOERTZEL, FOLDED, RESIDUE])
@pytest.mark.parametrize("amplitude,sigma", [(8000, 0), (8000, 2000), (300, 400), (32767, 2000)])
def test_stress_levels(A, O, torch, amplitude, sigma, method):
    run_case(A, O, A.FSK8_FREQS, W=500, seed=amplitude + sigma, amplitude=amplitude, sigma=sigma,
             method=method)
    if method != FOLDED:
        run_case(A, O, FSK8_ODD, W=500, seed=amplitude + sigma + 1, amplitude=amplitude,
                 sigma=sigma, method=method)


@pytest.mark.parametrize("method", [GOERTZEL, FOLDED, RESIDUE])
def test_zero_and_extreme_input(A, O, torch, method):
    n = 1024
    x = np.zeros((8, n), np.int16)
    x[1] = 32767
    x[2] = -32768
    x[3, ::2] = 32767
    x[3, 1::2] = -32768
    x[4] = np.where(np.sin(2 * np.pi * 32 * np.arange(n) / n) >= 0, 32767, -32768)
    x[5, 0] = 1
    x[6] = np.random.default_rng(0).integers(-32768, 32768, n)
    x[7] = np.round(32767 * np.cos(2 * np.pi * 64 * np.arange(n) / n))
    with A.Demodulator(freqs=A.FSK2_FREQS, method=method) as d:
        sym, mag = d.batch(x, mags=True)
    ref_sym, ref_P = O.goertzel(x, A.FSK2_FREQS, n)
    assert sym[0] == 0 and (mag[0] == 0).all()  # all-zero window: tie -> lowest index
    # These windows carry (almost) no energy at the tone bins, so max_k P_ref
    # is ~0 and "relative to max P" is ill-posed; normalise by the window's
    # spectral energy N*sum(x^2)/2 instead (equal to max P for a clean tone).
    xe = x.astype(np.float64)
    energy = n * (xe * xe).sum(axis=1) / 2
    denom = np.maximum(ref_P.max(axis=1), energy)
    err = (np.abs(mag[1:].astype(np.float64) - ref_P[1:]).max(axis=1) / denom[1:]).max()
    assert err <= MAG_TOL
    # Every symbol equals the double oracle's, including the windows whose
    # tone content is exactly zero or exactly tied: DC (rows 1, 2) and Nyquist
    # (row 3) put zero true power on both tones, the unit impulse (row 5)
    # exactly equal power; their fp32 margins are inside the error bound, so
    # the rescue decides them with the oracle's own double arithmetic
    # (DESIGN.md §2a). The energy scale lets a window whose fp32 tone powers
    # are exactly 0 pass as silence (tests/decision.py).
    n_band = check_decisions(sym, mag, ref_sym, ref_P, np.maximum(denom, 1e-30))
    assert n_band >= 4  # rows 0 (all zero), 1, 2, 3 and 5 are exact ties


@pytest.mark.parametrize("method", [GOERTZEL, RESIDUE])
def test_extreme_input_every_residue_class(A, O, torch, method):
    """Full-scale and degenerate windows through the residue classes (FSK8_ODD
    touches all four): magnitudes within the bar relative to the window's
    spectral energy, symbols equal wherever the oracle's decision is not a
    tie inside fp32 rounding."""
    n = 1024
    rng = np.random.default_rng(7)
    t = np.arange(n)
    x = np.zeros((12, n), np.int16)
    x[1] = 32767
    x[2, ::2] = 32767
    x[2, 1::2] = -32768
    x[3] = rng.integers(-32768, 32768, n)
    x[4] = np.where(np.sin(2 * np.pi * 41 * t / n) >= 0, 32767, -32768)
    for i, b in enumerate((50, 59, 68, 77, 86, 95)):
        x[5 + i] = np.clip(np.round(32767 * np.cos(2 * np.pi * b * t / n + i)
                                    + rng.normal(0, 3000, n)), -32768, 32767)
    x[11] = rng.integers(-32768, 32768, n) // 256
    with A.Demodulator(freqs=FSK8_ODD, method=method) as d:
        sym, mag = d.batch(x, mags=True)
    ref_sym, ref_P = O.goertzel(x, FSK8_ODD, n)
    xe = x.astype(np.float64)
    denom = np.maximum(np.maximum(ref_P.max(axis=1), n * (xe * xe).sum(axis=1) / 2), 1.0)
    assert (np.abs(mag.astype(np.float64) - ref_P).max(axis=1) / denom).max() <= MAG_TOL
    check_decisions(sym, mag, ref_sym, ref_P, denom)


@pytest.mark.parametrize("freqs,method", [("FSK8_FREQS", FOLDED), ("FSK8_ODD", RESIDUE),
                                          ("NONINT8", GOERTZEL)])
def test_ties_k8(A, O, torch, freqs, method):
    """window_sum.h decision rule (K = 8 kernels): an exact tie (the all-zero
    window: every power 0) goes to the lowest tone. A unit impulse puts
    exactly equal power x^2 on every tone too; the fp32 powers differ by
    ~1e-6 relative (rounding of the rotation constants, amplified by the
    recurrence), inside the error bound, so the rescue decides these windows
    with the oracle's double arithmetic and the symbol is the oracle's."""
    f = {"FSK8_FREQS": A.FSK8_FREQS, "FSK8_ODD": FSK8_ODD,
         "NONINT8": tuple(1234.5 + 1111.1 * i for i in range(8))}[freqs]
    n = 1024
    x = np.zeros((6, n), np.int16)
    for r, pos in enumerate((0, 1, 333, 1023)):
        x[r + 1, pos] = 12345 if r % 2 else -7
    with A.Demodulator(freqs=f, method=method) as d:
        assert d.method == method
        sym, mag = d.batch(x, mags=True)
    assert sym[0] == 0 and sym[5] == 0 and (mag[0] == 0).all() and (mag[5] == 0).all()
    ref_sym, ref_P = O.goertzel(x, f, n)
    for r in range(1, 5):
        assert np.abs(mag[r] / ref_P[r] - 1).max() <= MAG_TOL  # every tone at x^2
    # the impulse windows are exact mathematical ties, decided as the oracle does
    assert check_decisions(sym, mag, ref_sym, ref_P) >= 4


def test_device_pointers_and_async(A, O, torch):
    n, W = 1024, 2048
    pcm, truth = O.synth_fsk(A.FSK8_FREQS, n, W, 5)
    d_pcm = torch.from_numpy(pcm).cuda()
    d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
    d_mag = torch.empty((W, 8), dtype=torch.float32, device="cuda")
    with A.Demodulator(freqs=A.FSK8_FREQS) as d:
        assert d.batch_device(d_pcm, W, d_sym, d_mag) == W
        ref_sym, ref_P = O.goertzel(pcm, A.FSK8_FREQS, n)
        assert (d_sym.cpu().numpy() == ref_sym).all()
        assert rel_err(d_mag.cpu().numpy(), ref_P) <= MAG_TOL
        d_sym.zero_()
        s = torch.cuda.current_stream()
        d.batch_async(d_pcm, W, d_sym, None, stream=s.cuda_stream)
        s.synchronize()
        assert (d_sym.cpu().numpy() == ref_sym).all()


def test_gpu_synth_matches_cpu_generator(A, O, torch):
    for freqs, n, W, amp, sig in [(A.FSK2_FREQS, 1024, 513, 8000, 400),
                                  (A.FSK8_FREQS, 1024, 300, 8000, 2000),
                                  ((700.0, 1234.5, 9000.0), 256, 100, 32767, 2000)]:
        cfg = A.make_cfg(n=n, freqs=freqs)
        d_pcm = torch.empty((W, n), dtype=torch.int16, device="cuda")
        d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
        A.synth_fsk(cfg, 77, W, amp, sig, d_pcm, d_sym)
        torch.cuda.synchronize()
        pcm, sym = O.synth_fsk(freqs, n, W, 77, amp, sig)
        assert (d_pcm.cpu().numpy() == pcm).all()
        assert (d_sym.cpu().numpy() == sym).all()


@pytest.mark.parametrize("channels,mode", [(1, 0), (2, 0), (2, 1), (2, 2)])
def test_streaming_demodulate(A, O, torch, channels, mode):
    n = 1024
    L, _ = O.synth_fsk(A.FSK2_FREQS, n, 40, 11)
    R, _ = O.synth_fsk(A.FSK2_FREQS, n, 40, 12)
    if channels == 1:
        stream = L.reshape(-1)
    else:
        stream = np.stack([L.reshape(-1), R.reshape(-1)], axis=1).reshape(-1)
    # chunk as the receiver does: 60 ms Opus packets (2880 frames) plus ragged calls
    rng = np.random.default_rng(channels * 10 + mode)
    sizes = [2880, 2880, 1, 0, 1023, 1024, 1025, 7, 5000]
    ref = O.Stream(A.FSK2_FREQS, n=n, channels=channels, channel_mode=mode)
    got, want = [], []
    with A.Demodulator(freqs=A.FSK2_FREQS, channels=channels, channel_mode=mode) as d:
        pos = 0
        i = 0
        total_frames = stream.size // channels
        while pos < total_frames:
            fr = sizes[i] if i < len(sizes) else int(rng.integers(0, 4000))
            i += 1
            chunk = stream[pos * channels:(pos + fr) * channels]
            pos += fr
            got.append(d.demodulate(chunk))
            want.append(ref.push(chunk)[0])
            assert d.pending() == ref.pending()
    got = np.concatenate(got)
    want = np.concatenate(want)
    assert got.size == want.size == 40
    assert (got == want).all()


@pytest.mark.parametrize("channels,lead_in,hop", [(2, 312, 1024), (1, 312, 256), (2, 5000, 1024),
                                                  (1, 0, 1024)])
def test_streaming_lead_in(A, O, torch, channels, lead_in, hop):
    """cfg.lead_in drops the stream's first frames before windowing (the Opus
    decoder delay, DEMOD_OPUS_LOOKAHEAD = 312, OpusEncoder.kt:65-67): packets
    shorter and longer than the lead-in, demod_reset re-arms it, and the
    result equals the oracle's streaming restatement with the same skip."""
    n = 1024
    L, truth = O.synth_fsk(A.FSK8_FREQS, n, 30, 313 + channels)
    R, _ = O.synth_fsk(A.FSK8_FREQS, n, 30, 314 + channels)
    # the transmitter's symbols, delayed by lead_in samples of decoder output
    pre = np.random.default_rng(lead_in).integers(-3000, 3000, lead_in).astype(np.int16)
    mono = np.concatenate([pre, L.reshape(-1)])
    right = np.concatenate([pre[::-1], R.reshape(-1)])
    stream = mono if channels == 1 else np.stack([mono, right], axis=1).reshape(-1)
    sizes = [100, 200, 2880, 1, 7, 2880, 4000]
    for attempt in range(2):   # the second pass runs after demod_reset
        ref = O.Stream(A.FSK8_FREQS, n=n, hop=hop, channels=channels, lead_in=lead_in)
        got, want = [], []
        if attempt == 0:
            d = A.Demodulator(A.make_cfg(freqs=A.FSK8_FREQS, hop=hop, channels=channels,
                                         lead_in=lead_in))
        else:
            d.reset()
        pos, i = 0, 0
        total = mono.size
        while pos < total:
            fr = sizes[i % len(sizes)]
            i += 1
            chunk = stream[pos * channels:(pos + fr) * channels]
            pos += fr
            assert d.max_symbols(chunk.size // channels) >= 0
            got.append(d.demodulate(chunk))
            want.append(ref.push(chunk)[0])
            assert d.pending() == ref.pending()
        got, want = np.concatenate(got), np.concatenate(want)
        assert got.size == want.size == (30 * n - n) // hop + 1
        assert (got == want).all()
        if hop == n:
            assert (got == truth).all()   # aligned with the transmitted symbols
    d.close()


def test_streaming_buffer_too_small_consumes_nothing(A, torch):
    with A.Demodulator(freqs=A.FSK2_FREQS) as d:
        x = np.zeros(4096, np.int16)
        with pytest.raises(A.DemodError) as e:
            d.demodulate(x, max_symbols=3)
        assert e.value.code == A.DEMOD_BUFFER_TOO_SMALL
        assert d.pending() == 0
        assert d.demodulate(x).size == 4
        d.demodulate(x[:100])
        assert d.pending() == 100
        d.reset()
        assert d.pending() == 0


@pytest.mark.parametrize("freqs,method", [("FSK2_FREQS", GOERTZEL), ("FSK8_FREQS", FOLDED),
                                          ("FSK8_FREQS", GOERTZEL), ("FSK8_ODD", RESIDUE)])
def test_full_size_2e20_windows(A, O, torch, freqs, method):
    """Configs 2/3 at full size (2^20 windows, 2 GiB): every symbol equals the
    transmitted one (size-independent check), and a 4096-window sample equals
    the oracle bit-for-bit with magnitudes inside the tolerance."""
    f = FSK8_ODD if freqs == "FSK8_ODD" else getattr(A, freqs)
    n, W = 1024, 1 << 20
    cfg = A.make_cfg(n=n, freqs=f)
    d_pcm = torch.empty((W, n), dtype=torch.int16, device="cuda")
    d_true = torch.empty(W, dtype=torch.uint8, device="cuda")
    d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
    d_mag = torch.empty((W, len(f)), dtype=torch.float32, device="cuda")
    A.synth_fsk(cfg, A.BENCH_SEED, W, 8000, 400, d_pcm, d_true)
    torch.cuda.synchronize()
    cfg.method = method
    with A.Demodulator(cfg) as d:
        d.batch_device(d_pcm, W, d_sym, d_mag)
    assert torch.equal(d_sym, d_true)
    idx = np.sort(np.random.default_rng(3).choice(W, 4096, replace=False))
    ti = torch.from_numpy(idx).cuda()
    pcm = d_pcm[ti].cpu().numpy()
    ref_sym, ref_P = O.goertzel(pcm, f, n)
    assert (d_sym[ti].cpu().numpy() == ref_sym).all()
    assert rel_err(d_mag[ti].cpu().numpy(), ref_P) <= MAG_TOL
    del d_pcm


@pytest.mark.parametrize("name", ["fsk2_n1024", "fsk8_n1024", "k5_nonint_n512", "fsk2_hop256",
                                  "fsk4_n256_lowsnr"])
def test_golden_vectors_on_gpu(A, torch, name):
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"),
                allow_pickle=False)
    n, hop = int(g["n"]), int(g["hop"])
    freqs = tuple(g["freqs"])
    integer = all(abs(f * n / 48000.0 - round(f * n / 48000.0)) < 1e-9 for f in freqs)
    for method in (0, GOERTZEL) + ((RESIDUE,) if integer else ()):
        with A.Demodulator(n=n, hop=hop, freqs=freqs, method=method) as d:
            sym, mag = d.batch(g["pcm"], n_windows=g["sym"].size, mags=True)
        assert (sym == g["sym"]).all()
        assert rel_err(mag, g["P"]) <= MAG_TOL


def test_golden_stereo_stream_on_gpu(A, torch):
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "stereo_stream.npz"),
                allow_pickle=False)
    pf = int(g["packet_frames"])
    for mode in (0, 1, 2):
        with A.Demodulator(freqs=tuple(g["freqs"]), channels=2, channel_mode=mode) as d:
            out = [d.demodulate(g["pcm"][2 * i:2 * (i + pf)], mags=True)
                   for i in range(0, g["pcm"].size // 2, pf)]
            assert d.pending() == int(g[f"pending_mode{mode}"])
        sym = np.concatenate([o[0] for o in out])
        mag = np.concatenate([o[1] for o in out])
        assert (sym == g[f"sym_mode{mode}"]).all()
        assert rel_err(mag, g[f"P_mode{mode}"]) <= MAG_TOL


# ---- full-spectrum FFT detector (config 4) ---------------------------------


def _spec_err(spec, ref):
    return float((np.abs(spec.astype(np.float64) - ref).max(axis=1) / ref.max(axis=1)).max())


@pytest.mark.parametrize("freqs,hop,W", [("FSK2_FREQS", 1024, 1000), ("FSK8_FREQS", 1024, 777),
                                         ("FSK2_FREQS", 256, 200), ("FSK8_FREQS", 256, 130),
                                         ("FSK2_FREQS", 8, 3), ("FSK8_FREQS", 1000, 64)])
def test_fft_detector_matches_oracle(A, O, torch, freqs, hop, W):
    f = getattr(A, freqs)
    pcm, truth = O.synth_fsk(f, 1024, W, 31 + hop, 8000, 400)
    flat = pcm.reshape(-1)
    Wh = (flat.size - 1024) // hop + 1
    with A.Demodulator(freqs=f, hop=hop, method=FFT) as d:
        assert d.method == FFT
        sym, mag = d.batch(flat, n_windows=Wh, mags=True)
        # full spectrum on device
        d_pcm = torch.from_numpy(flat.copy()).cuda()
        d_sym = torch.empty(Wh, dtype=torch.uint8, device="cuda")
        d_spec = torch.empty((Wh, 513), dtype=torch.float32, device="cuda")
        d.batch_spectrum_async(d_pcm, Wh, d_sym, None, d_spec)
        torch.cuda.synchronize()
    ref_sym, ref_P = O.fft_demod(flat, f, 1024, hop)
    assert (sym == ref_sym).all()
    assert (d_sym.cpu().numpy() == ref_sym).all()
    assert rel_err(mag, ref_P) <= MAG_TOL
    # integer bins: the FFT detector computes the same |X_k|^2 as the Goertzel bank
    gs, gP = O.goertzel(flat, f, 1024, hop, Wh)
    assert (sym == gs).all()
    idx = np.arange(0, Wh, max(1, Wh // 64))
    full = np.stack([O.fft_power(flat[i * hop:i * hop + 1024]) for i in idx])
    assert _spec_err(d_spec.cpu().numpy()[idx], full) <= MAG_TOL
    if hop == 1024:
        assert (sym == truth).mean() > 0.999


def test_fft_detector_noninteger_tones_pick_nearest_bin(A, O, torch):
    f = (612.3, 2471.9, 5003.3, 9100.0, 15777.7)
    pcm, _ = O.synth_fsk(f, 1024, 300, 5, 8000, 400)
    with A.Demodulator(freqs=f, method=FFT) as d:
        sym, mag = d.batch(pcm, mags=True)
    ref_sym, ref_P = O.fft_demod(pcm, f, 1024)
    assert (sym == ref_sym).all()
    assert rel_err(mag, ref_P) <= MAG_TOL


@pytest.mark.parametrize("W", [1, 2, 3, 5, 66])
def test_fft_detector_sixteen_tones_small_batches(A, O, torch, W):
    """K = 16 (a whole 16-lane row in the quad layout's tone pick) and batches
    smaller than one 4-window group, with the full spectrum."""
    f = tuple(1000.0 + 1234.5 * i for i in range(16))
    pcm, _ = O.synth_fsk(f, 1024, W, 77 + W, 8000, 400)
    with A.Demodulator(freqs=f, method=FFT) as d:
        sym, mag = d.batch(pcm, mags=True)
        d_pcm = torch.from_numpy(pcm.reshape(-1).copy()).cuda()
        d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
        d_spec = torch.empty((W, 513), dtype=torch.float32, device="cuda")
        d.batch_spectrum_async(d_pcm, W, d_sym, None, d_spec)
        torch.cuda.synchronize()
    ref_sym, ref_P = O.fft_demod(pcm, f, 1024)
    assert (sym == ref_sym).all() and (d_sym.cpu().numpy() == ref_sym).all()
    assert rel_err(mag, ref_P) <= MAG_TOL
    full = np.stack([O.fft_power(pcm[i]) for i in range(W)])
    assert _spec_err(d_spec.cpu().numpy(), full) <= MAG_TOL


def test_fft_detector_extremes_and_streaming(A, O, torch):
    n = 1024
    x = np.zeros((5, n), np.int16)
    x[1] = 32767
    x[2, ::2] = 32767
    x[2, 1::2] = -32768
    x[3] = np.random.default_rng(9).integers(-32768, 32768, n)
    x[4] = np.round(32767 * np.cos(2 * np.pi * 64 * np.arange(n) / n))
    with A.Demodulator(freqs=A.FSK2_FREQS, method=FFT) as d:
        d_pcm = torch.from_numpy(x.reshape(-1).copy()).cuda()
        d_sym = torch.empty(5, dtype=torch.uint8, device="cuda")
        d_spec = torch.empty((5, 513), dtype=torch.float32, device="cuda")
        d.batch_spectrum_async(d_pcm, 5, d_sym, None, d_spec)
        torch.cuda.synchronize()
        spec = d_spec.cpu().numpy()
        assert (spec[0] == 0).all() and d_sym[0].item() == 0
        full = np.stack([O.fft_power(x[i]) for i in range(1, 5)])
        # DC and Nyquist carry all the energy in rows 1, 2: error relative to the peak bin
        assert _spec_err(spec[1:], full) <= MAG_TOL
        # streaming entry point through the FFT detector
        L, _ = O.synth_fsk(A.FSK8_FREQS, n, 12, 3)
    with A.Demodulator(freqs=A.FSK8_FREQS, method=FFT) as d:
        got = np.concatenate([d.demodulate(L.reshape(-1)[i:i + 2880])
                              for i in range(0, L.size, 2880)])
    ref, _ = O.fft_demod(L.reshape(-1), A.FSK8_FREQS, n)
    assert (got == ref).all()


@pytest.mark.parametrize("method,hop", [(GOERTZEL, 1024), (GOERTZEL, 256), (FOLDED, 512),
                                        (RESIDUE, 1024), (2, 256)])
def test_host_batch_multi_chunk(A, O, torch, method, hop):
    """Host-pointer demod_batch streams its input in 65536-window chunks over
    two device slots (demod_api.cpp run_host). Across chunk boundaries (and
    the n - hop overlap of sliding windows) its output must equal the
    device-pointer path on the same samples bit-for-bit, and a sample of
    windows must match the oracle."""
    n = 1024
    f = A.FSK8_FREQS if method == FOLDED else FSK8_ODD if method == RESIDUE else A.FSK2_FREQS
    Wsrc = 3 * 65536 // (n // hop) + 37           # source windows of n samples
    cfg = A.make_cfg(n=n, freqs=f)
    d_src = torch.empty((Wsrc, n), dtype=torch.int16, device="cuda")
    d_true = torch.empty(Wsrc, dtype=torch.uint8, device="cuda")
    A.synth_fsk(cfg, A.BENCH_SEED + hop, Wsrc, 8000, 400, d_src, d_true)
    torch.cuda.synchronize()
    W = (Wsrc * n - n) // hop + 1
    assert W > 3 * 65536
    d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
    d_mag = torch.empty((W, len(f)), dtype=torch.float32, device="cuda")
    flat = d_src.cpu().numpy().reshape(-1)
    with A.Demodulator(n=n, hop=hop, freqs=f, method=method) as d:
        assert d.method == method
        d.batch_device(d_src, W, d_sym, d_mag)
        sym, mag = d.batch(flat, n_windows=W, mags=True)
        sym2 = d.batch(flat, n_windows=W)   # second call reuses the slots
    assert np.array_equal(sym, d_sym.cpu().numpy())
    assert np.array_equal(sym2, sym)
    assert np.array_equal(mag, d_mag.cpu().numpy())
    idx = np.array([0, 1, 65535, 65536, 65537, 131071, 131072, W - 2, W - 1])
    win = np.stack([flat[i * hop:i * hop + n] for i in idx])
    oracle = O.fft_demod if method == 2 else O.goertzel
    ref_sym, ref_P = oracle(win.reshape(-1), f, n, n)
    assert (sym[idx] == ref_sym).all()
    assert rel_err(mag[idx], ref_P) <= MAG_TOL


@pytest.mark.parametrize("n_streams,n,bits,max_payload", [
    (1, 1, 1, 4096), (3, 2048, 1, 4096), (128, 2048, 3, 4096), (5, 40000, 1, 4096),
    (4, 32769, 1, 4096), (7, 10923, 3, 4096), (2, 9000, 4, 4096), (3, 4097, 8, 4096),
    (6, 1000, 2, 17), (2, 300, 3, 1), (1, 0, 1, 4096), (0, 100, 1, 4096)])
def test_device_framing_matches_host_codec(A, torch, n_streams, n, bits, max_payload):
    """demod_frame_streams_async frames every stream byte-for-byte as the host
    codec demod_frame_symbols (itself pinned to the reference's nanopb in
    test_frame.py), and the frames decode back to the symbols."""
    rng = np.random.default_rng(n_streams * 7919 + n + bits)
    # values above the symbol width are masked, as demod_pack_symbols does
    sym = rng.integers(0, 256, (n_streams, n), dtype=np.uint8)
    stride = A.frame_symbols_size(n, bits, max_payload)
    d_sym = torch.from_numpy(sym.copy()).cuda() if sym.size else torch.zeros(1, dtype=torch.uint8,
                                                                              device="cuda")
    d_out = torch.full((max(n_streams * stride, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    got = A.frame_streams_async(d_sym, n_streams, n, bits, d_out, max_payload)
    torch.cuda.synchronize()
    assert got == stride
    out = d_out.cpu().numpy()
    mask = (1 << bits) - 1
    for s in range(n_streams):
        ref = A.frame_symbols(sym[s], bits, max_payload)
        assert out[s * stride:(s + 1) * stride].tobytes() == ref
        if n:
            per = max_payload * 8 // bits
            back, got_n = [], 0
            for payload in A.iter_frames(ref):
                cnt = min(per, n - got_n)
                back.append(A.unpack_symbols(payload, cnt, bits))
                got_n += cnt
            assert np.array_equal(np.concatenate(back), sym[s] & mask)


@pytest.mark.parametrize("plan", ["fold", "odd"])
@pytest.mark.parametrize("mode", ["bursts", "slices"])
def test_batch_launch_slices(A, O, torch, monkeypatch, mode, plan):
    """Batches whose symbol + magnitude output exceeds ~10 MiB run as one
    launch that writes each XCD's L2 back in bursts (round 3, the default) or,
    with FSKD_WB_BURSTS=0 (read at create), as several launch slices
    (demod_batch_launches); either must give the same symbols and powers as one
    launch over the same windows (smaller batches below the threshold),
    including a window count that is not a multiple of the slice. Plans: the
    configs[2] tones (fold detector) and integer bins 32 + 9 i (residue
    detector)."""
    if mode == "slices":
        monkeypatch.setenv("FSKD_WB_BURSTS", "0")
    else:
        monkeypatch.delenv("FSKD_WB_BURSTS", raising=False)
    n, W = 1024, (1 << 20) + 77
    f = A.FSK8_FREQS if plan == "fold" else tuple(48000.0 * (32 + 9 * i) / n for i in range(8))
    cfg = A.make_cfg(n=n, freqs=f)
    d_pcm = torch.empty((W, n), dtype=torch.int16, device="cuda")
    A.synth_fsk(cfg, 99, W, 8000, 400, d_pcm)
    sym = torch.empty(W, dtype=torch.uint8, device="cuda")
    mag = torch.empty((W, 8), dtype=torch.float32, device="cuda")
    with A.Demodulator(cfg) as d:
        # detector launches, + the rescue launch for the residue detector's
        # plans (round 5: pass 0 by the residue fold lives there); the fold
        # detector re-decides its flagged windows inside its own kernel
        r = 1 if plan == "odd" else 0
        assert d.batch_launches(W, mags=True) == (4 if mode == "slices" else 1) + r
        assert d.batch_launches(W, mags=False) == 1 + r
        assert d.batch_launches(1 << 18, mags=True) == 1 + r
        d.batch_device(d_pcm, W, sym, mag)
        ref_sym = torch.empty_like(sym)
        ref_mag = torch.empty_like(mag)
        step = 1 << 18                       # below the threshold: one launch each
        for w0 in range(0, W, step):
            c = min(step, W - w0)
            d.batch_device(d_pcm[w0:w0 + c], c, ref_sym[w0:w0 + c], ref_mag[w0:w0 + c])
    torch.cuda.synchronize()
    assert torch.equal(sym, ref_sym)
    assert torch.equal(mag.view(torch.int32), ref_mag.view(torch.int32))
    with A.Demodulator(freqs=A.FSK2_FREQS) as d:
        # 9 MiB: one launch, and the 2-FSK plain bank rescues in the kernel
        assert d.batch_launches(1 << 20, mags=True) == 1
    # the rescue launch remains for segment-shared windows and n != 1024
    with A.Demodulator(A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS)) as d:
        assert d.slide_windows > 0 and d.batch_launches(1 << 16, mags=True) == 2
    with A.Demodulator(A.make_cfg(n=256, hop=256, freqs=(1500.0, 3000.0))) as d:
        assert d.batch_launches(1 << 16, mags=True) == 2
    with A.Demodulator(A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS, method=A.METHOD_FFT)) as d:
        assert d.batch_launches(1 << 16, mags=True) == 1


# ---- GPU against the reference's own FFT at N = 1024 -------------------------
# tests/golden/ref_kissfft.npz holds opus_fft_c outputs of the reference's
# kiss_fft.c (CUSTOM_MODES build, oracle/kissfft_custom_harness.c) for 14
# seeded 1024-sample frames. Its powers are Q15 fixed point: errors scale with
# the frame's energy, so the bar is 3e-4 of the Parseval total N * sum(x^2)
# (tests/test_oracle.py REF_FFT_TOL), far looser than the 1e-5 oracle bar the
# other tests hold; this pins the GPU path to reference code directly.
REF_FFT_TOL = 3e-4


def _ref1024():
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_kissfft.npz"),
                allow_pickle=False)
    x = g["x1024"]
    Y = (g["re1024"] + 1j * g["im1024"]) * 1024 / 2.0 ** int(g["preshift"])
    energy = 1024 * (x.astype(np.float64) ** 2).sum(axis=1)
    return x, np.abs(Y[:, :513]) ** 2, np.maximum(energy, 1.0)


def test_fft_detector_spectrum_vs_reference_kissfft(A, torch):
    x, Pr, energy = _ref1024()
    W = len(x)
    with A.Demodulator(freqs=A.FSK2_FREQS, method=FFT) as d:
        d_pcm = torch.from_numpy(x.reshape(-1).copy()).cuda()
        d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
        d_spec = torch.empty((W, 513), dtype=torch.float32, device="cuda")
        d.batch_spectrum_async(d_pcm, W, d_sym, None, d_spec)
        torch.cuda.synchronize()
    spec = d_spec.cpu().numpy().astype(np.float64)
    err = np.abs(spec - Pr).max(axis=1) / energy
    assert err.max() <= REF_FFT_TOL, err
    # the 2-FSK frames (rows 0-3): the symbol is the reference spectrum's argmax
    assert (d_sym.cpu().numpy()[:4] == np.argmax(Pr[:4][:, [32, 64]], axis=1)).all()


@pytest.mark.parametrize("method", [GOERTZEL, FOLDED, RESIDUE, 0])
@pytest.mark.parametrize("plan", ["fsk2", "fsk8"])
def test_tone_bank_vs_reference_kissfft(A, method, plan, torch):
    """Every Goertzel-family detector's |X_k|^2 at the tone bins against the
    reference kiss FFT's bins, and its symbols on the FSK frames against the
    reference spectrum's argmax over the tone bins."""
    x, Pr, energy = _ref1024()
    if plan == "fsk2":
        freqs, bins, rows = A.FSK2_FREQS, [32, 64], slice(0, 4)
    else:
        freqs, bins, rows = A.FSK8_FREQS, [32 + 8 * i for i in range(8)], slice(4, 8)
    with A.Demodulator(freqs=freqs, method=method) as d:
        sym, mag = d.batch(x.reshape(-1), mags=True)
    err = np.abs(mag.astype(np.float64) - Pr[:, bins]).max(axis=1) / energy
    assert err.max() <= REF_FFT_TOL, err
    assert (sym[rows] == np.argmax(Pr[rows][:, bins], axis=1)).all()


@pytest.mark.parametrize("W", [1, 3, 4, 5, 7, 257, 4097])
@pytest.mark.parametrize("hop", [1024, 256])
def test_fft_spectrum_store_paths_agree(A, O, torch, W, hop):
    """The full-spectrum store has two paths: a 16-byte-aligned output goes
    through the linear power slab and leaves as 16-byte stores of the group's
    contiguous run (partial last group: scalar tail), any other alignment
    through the quad_slot slab with dword stores. Both carry the same powers:
    equal bits, and equal to the oracle's spectrum on a sample."""
    n = 1024
    src = (W - 1) * hop // n + 2
    pcm, _ = O.synth_fsk(A.FSK8_FREQS, n, src, 31 + W, 8000, 400)
    flat = pcm.reshape(-1)
    Wh = min(W, (flat.size - n) // hop + 1)
    d_pcm = torch.from_numpy(flat.copy()).cuda()
    with A.Demodulator(freqs=A.FSK8_FREQS, hop=hop, method=FFT) as d:
        outs = []
        for off in (0, 1):   # off 1: the spectrum 4 bytes past a 16-byte boundary
            buf = torch.full((Wh * 513 + 8,), -1.0, dtype=torch.float32, device="cuda")
            spec = buf[off:off + Wh * 513]
            d_sym = torch.empty(Wh, dtype=torch.uint8, device="cuda")
            d_mag = torch.empty((Wh, 8), dtype=torch.float32, device="cuda")
            d.batch_spectrum_async(d_pcm, Wh, d_sym, d_mag, spec)
            torch.cuda.synchronize()
            b = buf.cpu().numpy()
            assert (b[:off] == -1.0).all() and (b[off + Wh * 513:] == -1.0).all()
            outs.append((d_sym.cpu().numpy(), d_mag.cpu().numpy(), spec.cpu().numpy()))
    (s0, m0, p0), (s1, m1, p1) = outs
    assert np.array_equal(s0, s1) and np.array_equal(m0.view(np.uint32), m1.view(np.uint32))
    assert np.array_equal(p0.view(np.uint32), p1.view(np.uint32))
    spec = p0.reshape(Wh, 513)
    idx = np.unique(np.concatenate([np.arange(min(Wh, 8)), np.arange(max(0, Wh - 8), Wh)]))
    full = np.stack([O.fft_power(flat[i * hop:i * hop + n]) for i in idx])
    assert _spec_err(spec[idx], full) <= MAG_TOL
    ref_sym, ref_P = O.fft_demod(flat, A.FSK8_FREQS, n, hop)
    assert (s0 == ref_sym[:Wh]).all()
    assert rel_err(m0, ref_P[:Wh]) <= MAG_TOL
