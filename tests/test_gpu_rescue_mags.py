"""The magnitudes the decision rescue writes, and the windows of the
segment-shared kernels that start off a multiple of n, held to the sentences
of include/demod.h that promise them — bit for bit, or within the derived
bound (demod_error_model) plus half an fp32 ulp. No measured tolerance.

  test_shared_windows_equal_windows_alone, test_fsk2_fold_pass0_alone
      DEMOD_METHOD_GOERTZEL / DEMOD_METHOD_FOLDED: at n = 1024, hop = 64 H < n
      "same results as evaluating each window alone" (and demod_slide_windows:
      "The results are the same either way"). EVERY window x[w hop : w hop +
      n] of a stream goes, cut out, through a handle at hop = n with the same
      plan and forced method: same symbols and the same magnitude bits,
      flagged or not, at every tile position (rotation row, carried folded
      sums, shared segment states of a run).
  test_pass0_magnitudes_within_derived_bound
      "each form with its own derived bound against the definition's, so the
      rewritten powers are within that bound of the definition's" and
      demod_error_model's |sqrt(P_first,k) - sigma(P_oracle,k)| <= rho_first
      sqrt(sum x^2): the rescue launch's first pass by shared segment states,
      by the fold, by the residue fold, and the FFT's at its tone bins.
  test_exact_chain_bits_on_shared_windows, test_exact_chain_bits_other_lengths
      "with the definition's own arithmetic (powers bit-identical to it; every
      rescued window with FSKD_RESCUE_SEG=0)" and demod_rescue_tau64: "0:
      every flagged window takes the exact path — n != 1024,
      FSKD_RESCUE_SEG=0": the oracle's powers rounded to fp32, bit for bit.

Signal (tests/error_model.py mixed_stream_windows): runs of 1..40 windows
of near ties beside runs of clean FSK at sigma 400, so every 512-window chunk
of the rescue launch sees dense runs, sparse runs and runs cut by its end,
and W = 512 + 77 leaves a partial chunk and a partial last tile. The near-tie
runs tie in EVERY window (tie_run), not only in those that start a block:
with the blocks of `two_tone_equal` the plain 2-FSK plan has no near tie off
a multiple of n at all, and the off-bin plans none anywhere.

`sure` windows (guards.sure_mask: oracle top-2 margin below half the flag
threshold) are flagged whatever the fp32 rounding does, hence rescued: the
assertions about rescued powers are made on them, and a second handle under
FSKD_NO_RESCUE=flags shows bit 7 on every one. The fixture conditions
(guards.rescue_fixture: 32 sure windows, 8 of them off a multiple of n, a run
of 8 consecutive ones, 32 windows that are never flagged) need the oracle and
the error model only; test_fixture_conditions checks them without a device.
"""
import json
import zlib

import numpy as np
import pytest

import error_model as EM
import guards as G
from decision import check_decisions
from gpu_support import torch  # noqa: F401

gpu = pytest.mark.gpu

AUTO, GOERTZEL, FFT, FOLDED, RESIDUE = 0, 1, 2, 3, 4
N = 1024
W = 512 + 77            # one full chunk of the rescue launch and a partial one
BIN = EM.BIN
FOLD16 = tuple(BIN * 8 * (2 + i) for i in range(16))          # multiples of 8 bins
PLANS = {
    "FSK2_FREQS": (1500.0, 3000.0),
    "FSK8_FREQS": tuple(1500.0 + 375.0 * i for i in range(8)),   # fold by 16
    "NONINT3": (1234.5, 2345.6, 4321.0),
    "REINSCH2": (30.0, 23950.0),                                 # |sin w| < 0.1: the Reinsch recurrence
    "K16": tuple(BIN * (20 + 7 * i) for i in range(16)),
    "FSK8_ODD": tuple(BIN * (32 + 9 * i) for i in range(8)),
    "K3": tuple(BIN * b for b in (40, 64, 120)),                 # generic fold, odd K
    "FOLD12": FOLD16[:12],                                       # pass 0 by the fold (K <= 12)
    "FOLD13": FOLD16[:13],                                       # above it: by segments
    "FOLD16": FOLD16,
    "FFT_ODD": tuple(BIN * (33 + 7 * i) for i in range(4)),
    "ODD8": tuple(BIN * (32 + 9 * i) for i in range(8)),         # residues 0 .. 7
    "EDGES4": (1 * BIN, 2 * BIN, 511 * BIN, 510 * BIN),          # residues 1, 2, 7, 6
}

# (plan, method, hop): the segment-shared handles
SLIDE = ([("FSK2_FREQS", GOERTZEL, 64 * H) for H in range(1, 16)] +
         [(p, GOERTZEL, 64 * H) for p in ("NONINT3", "REINSCH2", "K16", "FSK8_ODD") for H in (1, 4, 7, 15)] +
         [(p, FOLDED, 64 * H) for p in ("FSK8_FREQS", "K3") for H in range(1, 16)] +
         [(p, FOLDED, 64 * H) for p in ("FOLD12", "FOLD13") for H in (1, 4)])
# test_gpu_rescue_launch.py test_pass0_forms' table: every form of the first
# pass, in the detector kernel at hop = n and in the rescue launch at hop 256
FORMS = [(p, m, hop) for p, m in (("FOLD12", FOLDED), ("FOLD13", FOLDED), ("FOLD16", FOLDED), ("FOLD16", FFT),
                                  ("FOLD12", FFT), ("FFT_ODD", FFT), ("ODD8", RESIDUE), ("EDGES4", RESIDUE),
                                  ("FOLD16", RESIDUE))
         for hop in (1024, 256)]
EXACT = [c for c in SLIDE if c[2] // 64 in (1, 4, 7, 15)]


def case_id(c):
    return f"{c[0]}-m{c[1]}-hop{c[2]}"


def case_env(case):
    """At K <= 2 on multiples of 8 bins the direct kernel takes pass 0 by the
    fold and the rescue launch by segments: FSKD_PASS0_FOLD=0 puts both on
    segments (tests/test_gpu_error_model.py
    test_rescue_launch_equals_in_kernel_rescue)."""
    return (("FSKD_PASS0_FOLD", "0"),) if case[0] == "FSK2_FREQS" and case[1] == GOERTZEL else ()


_FIXTURES = {}


def fixture(A, O, case, env=()):
    """The case's stream, its oracle results and window classes, computed once
    and shared (read-only) by the tests on it; asserts the fixture conditions."""
    key = (case, env)
    if key not in _FIXTURES:
        plan, method, hop = case
        freqs = PLANS[plan]
        total = (W - 1) * hop + N
        x = EM.mixed_stream_windows(freqs, -(-total // N), zlib.crc32(case_id(case).encode()), hop)[:total]
        cfg = A.make_cfg(n=N, hop=hop, freqs=freqs, method=method)
        with G.env(**dict(env)):
            model = A.error_model(cfg)
            info = A.plan_info(cfg)
        assert info["method"] == method and model["rho_first"] > 0
        ref_sym, ref_P = (O.fft_demod if method == FFT else O.goertzel)(x, freqs, N, hop=hop, fs=EM.FS,
                                                                     threads=16)
        ref_sym, ref_P = ref_sym[:W], ref_P[:W]
        fx = G.rescue_fixture(model, x, N, hop, W, ref_P)
        xw = fx.pop("xw")
        fx.update(case=case, freqs=freqs, cfg=cfg, model=model, info=info, x=x, ref_sym=ref_sym, ref_P=ref_P,
                  e_raw=(xw * xw).sum(axis=1))
        for v in fx.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FIXTURES[key] = fx
    return _FIXTURES[key]


def device_run(A, fx, env=()):
    """The case's handle over its stream, once per environment: symbols and
    magnitudes, the symbols of a call without magnitudes, and the flags of a
    second handle with the rescue's flags kept and the rescue off."""
    key = ("run", env)
    if key not in fx:
        x, cfg = fx["x"], fx["cfg"]
        slide = fx["case"][2] < N and fx["case"][1] in (GOERTZEL, FOLDED)
        with G.env(**dict(env)), A.Demodulator(cfg) as d:
            assert d.method == fx["case"][1]
            assert (d.slide_windows > 0) == slide
            assert d.rescue_tau64 > 0
            assert d.rescue_tau == pytest.approx(fx["model"]["tau"], rel=1e-12)
            assert d.rescue_tau64 == pytest.approx(fx["model"]["tau64"], rel=1e-12)
            sym, mag = d.batch(x, n_windows=W, mags=True)
            sym0 = d.batch(x, n_windows=W)
        with G.env(FSKD_NO_RESCUE="flags", **dict(env)), A.Demodulator(cfg) as d:
            flags = d.batch(x, n_windows=W)
        sure = fx["sure"]
        missed = np.flatnonzero(sure & ((flags & 0x80) == 0))
        assert missed.size == 0, ("sure windows not flagged", missed[:8].tolist())
        assert ((flags & 0x80) == 0).sum() >= 32
        assert np.array_equal(sym0, sym), "symbols depend on whether magnitudes are requested"
        fx[key] = {"sym": sym, "mag": mag, "flagged": (flags & 0x80) != 0}
    return fx[key]


def report(test, fx, r, **more):
    """One line of counts per case (information, not asserted)."""
    flagged = r["flagged"] if r is not None else None
    row = {"test": test, "case": case_id(fx["case"]) if "case" in fx else fx["id"], "windows": int(fx["sure"].size),
           "sure": int(fx["sure"].sum()), "sure_off_n": int((fx["sure"] & fx["off"]).sum()),
           "off_n": int(fx["off"].sum())}
    if flagged is not None:
        row.update(flagged=int(flagged.sum()), unflagged=int((~flagged).sum()))
    row.update(more)
    print("\nRESCUE_MAGS " + json.dumps(row))


def alone_run(A, fx, env=()):
    """Every window of the case's stream cut out and laid end to end: a
    hop = n stream of W windows through a handle with the same plan and
    method, each window evaluated alone."""
    plan, method, hop = fx["case"]
    alone = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(fx["x"], N)[::hop][:W])
    assert alone.shape == (W, N)
    with G.env(**dict(env)), A.Demodulator(A.make_cfg(n=N, hop=N, freqs=fx["freqs"], method=method)) as d:
        assert d.method == method and d.slide_windows == 0
        return d.batch(alone, mags=True)


def diff_windows(a, b):
    return np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))


# ---- 1. every segment-shared window equals the same window evaluated alone

@gpu
@pytest.mark.parametrize("case", SLIDE, ids=case_id)
def test_shared_windows_equal_windows_alone(A, O, torch, case):
    """demod.h: "same results as evaluating each window alone". Symbols and
    magnitude bits of EVERY window, flagged or not, at every tile position."""
    env = case_env(case)
    fx = fixture(A, O, case, env)
    r = device_run(A, fx, env)
    sym_a, mag_a = alone_run(A, fx, env)
    report("alone", fx, r)
    bad = np.flatnonzero(r["sym"] != sym_a)
    assert bad.size == 0, ("symbols differ from the window alone", bad[:8].tolist())
    bad = diff_windows(r["mag"], mag_a)
    assert bad.size == 0, ("magnitude bits differ from the window alone", bad.size, bad[:8].tolist(),
                           r["flagged"][bad[:8]].tolist(), r["mag"][bad[:2]].tolist(), mag_a[bad[:2]].tolist())


@gpu
@pytest.mark.parametrize("H", list(range(1, 16)))
def test_fsk2_fold_pass0_alone(A, O, torch, H):
    """The shipped 2-FSK configuration (no switch): the window alone takes its
    first pass by the fold, the shared one by segments — two forms, each
    within its own bound — so flagged windows may differ in magnitude bits;
    the symbols and the unflagged windows' bits must not."""
    fx = fixture(A, O, ("FSK2_FREQS", GOERTZEL, 64 * H))
    r = device_run(A, fx)
    sym_a, mag_a = alone_run(A, fx)
    assert np.array_equal(r["sym"], sym_a)
    keep = ~r["flagged"]
    bad = diff_windows(r["mag"][keep], mag_a[keep])
    assert bad.size == 0, ("unflagged magnitude bits differ", np.flatnonzero(keep)[bad[:8]].tolist())


# ---- 2. the rescue launch's pass 0 within its derived bound

@gpu
@pytest.mark.parametrize("case", SLIDE + FORMS, ids=case_id)
def test_pass0_magnitudes_within_derived_bound(A, O, torch, case):
    """demod_error_model: |sqrt(P_first,k) - sigma(P_oracle,k)| <= rho_first
    sqrt(sum x^2), the stored power rounded to fp32 (half an ulp: 2^-24
    relative in P, so 2^-24 sqrt(P) covers sqrt P) — on every sure window and
    every tone; and the decision rule on all windows."""
    env = case_env(case)
    fx = fixture(A, O, case, env)
    r = device_run(A, fx, env)
    sure = fx["sure"]
    g = r["mag"][sure].astype(np.float64)
    bound = fx["model"]["rho_first"] * np.sqrt(fx["e_raw"][sure])[:, None] + 2.0 ** -24 * np.sqrt(g)
    err = np.abs(np.sqrt(g) - EM.sigma(fx["ref_P"][sure]))
    ratio = err / bound
    exact = int((r["mag"][sure].view(np.uint32) ==
                 fx["ref_P"][sure].astype(np.float32).view(np.uint32)).all(axis=1).sum())
    report("pass0", fx, r, worst_ratio=float(ratio.max()), sure_with_oracle_bits=exact,
           fold64=int(fx["info"]["fold64"]))
    bad = np.flatnonzero((err > bound).any(axis=1))
    assert bad.size == 0, ("outside rho_first sqrt(sum x^2) + half an ulp", bad.size,
                           np.flatnonzero(sure)[bad[:8]].tolist(), float(ratio.max()))
    check_decisions(r["sym"], r["mag"], fx["ref_sym"], fx["ref_P"])


# ---- 3. the exact chain's bits, wherever it is the only rescue

@gpu
@pytest.mark.parametrize("case", EXACT, ids=case_id)
def test_exact_chain_bits_on_shared_windows(A, O, torch, case):
    """FSKD_RESCUE_SEG=0: "every flagged window takes the exact path": each
    sure window's magnitudes are the oracle's powers rounded to fp32, bit for
    bit, and the symbols are those of the run with the first pass on."""
    env = case_env(case)
    fx = fixture(A, O, case, env)
    r = device_run(A, fx, env)
    with G.env(FSKD_RESCUE_SEG="0", **dict(env)), A.Demodulator(fx["cfg"]) as d:
        assert d.slide_windows > 0
        assert d.rescue_tau64 == 0.0
        sym_x, mag_x = d.batch(fx["x"], n_windows=W, mags=True)
    sure = fx["sure"]
    report("exact_slide", fx, r)
    assert np.array_equal(sym_x, r["sym"])
    bad = diff_windows(mag_x[sure], fx["ref_P"][sure].astype(np.float32))
    assert bad.size == 0, ("not the oracle's bits", bad.size, np.flatnonzero(sure)[bad[:8]].tolist())
    check_decisions(sym_x, mag_x, fx["ref_sym"], fx["ref_P"])


def plan_at(kind, n):
    """2-FSK on the plain bank; error_model.CASES' fold_n256 / fold_n4096 and
    residue_n256 / residue_n4096 plans carried to window length n: up to eight
    tones on multiples of 8 bins, five or eight integer bins over the residue
    classes."""
    f = EM.FS / n
    if kind == "plain":
        return GOERTZEL, (1500.0, 3000.0)
    if kind == "fold":
        return FOLDED, tuple(f * 8 * (2 + i) for i in range(min(8, n // 16 - 2)))
    if n >= 512:
        return RESIDUE, tuple(f * (n // 32 + 9 * i) for i in range(8))
    return RESIDUE, tuple(f * (n // 32 + 3 * i) for i in range(5))


LENGTHS = [(kind, n, hop) for kind in ("plain", "fold", "residue") for n in (64, 256, 512, 2048, 4096)
           for hop in (n, n // 4)]


def pool_size(n):
    """Near-tie windows per stream (guards.near_tie_windows): 256; at n = 64,
    where int16 rounding moves a window's margin by as much as the fold
    detector's threshold and one window in 15 stays sure, 768 (of 64 samples
    each)."""
    return 768 if n == 64 else 256


TIE_RUNS, TIE_BLOCKS, CLEAN_BLOCKS = 8, 10, 40


def length_fixture(A, O, case):
    """pool_size(n) near-tie windows of length n end to end (hop = n / 4: the
    windows between them are whatever falls out, hardly ever a near tie), then
    TIE_RUNS runs of TIE_BLOCKS n samples of error_model.tie_run, each its own
    tone pair and phases (every window inside a run ties wherever it starts:
    the sure windows off a multiple of n, consecutive), then CLEAN_BLOCKS
    symbols of clean FSK at sigma 400 (never flagged); the oracle's results
    and the window classes, under the same fixture conditions as at n = 1024
    (guards.rescue_fixture)."""
    if case not in _FIXTURES:
        kind, n, hop = case
        method, freqs = plan_at(kind, n)
        name = f"{kind}-n{n}-hop{hop}"
        seed = zlib.crc32(name.encode())
        rng = np.random.default_rng(seed)
        x = np.concatenate([G.near_tie_windows(freqs, pool_size(n), seed, n=n)[0].reshape(-1)] +
                           [EM.tie_run(freqs, n, TIE_BLOCKS * n, rng) for _ in range(TIE_RUNS)] +
                           [O.synth_fsk(freqs, n, CLEAN_BLOCKS, seed, 8000, 400, fs=EM.FS)[0].reshape(-1)])
        Wn = (x.size - n) // hop + 1
        cfg = A.make_cfg(n=n, hop=hop, freqs=freqs, method=method)
        model, info = A.error_model(cfg), A.plan_info(cfg)
        assert info["method"] == method and info["slide"] == 0
        assert model["rho_first"] == 0 and model["tau"] > 0
        ref_sym, ref_P = O.goertzel(x, freqs, n, hop=hop, fs=EM.FS, threads=16)
        ref_sym, ref_P = ref_sym[:Wn], ref_P[:Wn]
        fx = G.rescue_fixture(model, x, n, hop, Wn, ref_P)
        del fx["xw"]
        fx.update(id=name, x=x, W=Wn, cfg=cfg, model=model, ref_sym=ref_sym, ref_P=ref_P)
        _FIXTURES[case] = fx
    return _FIXTURES[case]


@gpu
@pytest.mark.parametrize("case", LENGTHS, ids=lambda c: f"{c[0]}-n{c[1]}-hop{c[2]}")
def test_exact_chain_bits_other_lengths(A, O, torch, case):
    """n != 1024: no first pass (rescue_tau64 = 0), the rescue is a launch of
    its own and the exact chain is all of it: each sure window's magnitudes
    are the oracle's powers rounded to fp32, bit for bit."""
    fx = length_fixture(A, O, case)
    x, Wn, sure = fx["x"], fx["W"], fx["sure"]
    with A.Demodulator(fx["cfg"]) as d:
        assert d.method == fx["cfg"].method and d.slide_windows == 0
        assert d.rescue_tau64 == 0.0
        assert d.rescue_tau == pytest.approx(fx["model"]["tau"], rel=1e-12)
        assert d.batch_launches(Wn, True) == 2
        sym, mag = d.batch(x, n_windows=Wn, mags=True)
    with G.env(FSKD_NO_RESCUE="flags"), A.Demodulator(fx["cfg"]) as d:
        flags = d.batch(x, n_windows=Wn)
    flagged = (flags & 0x80) != 0
    report("exact_lengths", fx, {"flagged": flagged})
    assert flagged[sure].all(), np.flatnonzero(sure & ~flagged)[:8].tolist()
    assert (~flagged).sum() >= 32
    bad = diff_windows(mag[sure], fx["ref_P"][sure].astype(np.float32))
    assert bad.size == 0, ("not the oracle's bits", bad.size, np.flatnonzero(sure)[bad[:8]].tolist())
    check_decisions(sym, mag, fx["ref_sym"], fx["ref_P"])


# ---- the fixture conditions: the oracle and the error model alone, no device

@pytest.mark.parametrize("case", SLIDE + FORMS, ids=case_id)
def test_fixture_conditions(A, O, case):
    """Every stream of the tests above holds what they stand on: fixture()
    asserts it in guards.rescue_fixture (32 sure windows, 8 of them off a
    multiple of n where hop < n, a run of 8 consecutive sure windows, 32
    windows no detector flags). No window is in both classes."""
    fx = fixture(A, O, case, case_env(case))
    assert not (fx["sure"] & fx["clear"]).any()


@pytest.mark.parametrize("case", LENGTHS, ids=lambda c: f"{c[0]}-n{c[1]}-hop{c[2]}")
def test_fixture_conditions_other_lengths(A, O, case):
    """The same conditions on the streams at n != 1024 (length_fixture)."""
    fx = length_fixture(A, O, case)
    assert not (fx["sure"] & fx["clear"]).any()
