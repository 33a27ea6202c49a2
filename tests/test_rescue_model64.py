"""The in-kernel rescue's first pass (rescue_rows.h rescue_rows, pass 0),
its derived error bound checked on the CPU.

Pass 0 re-computes a flagged window's K tone powers in double the way the
fp32 plain bank computes them: each of the row's 16 lanes runs every tone's
recurrence over its own 64 samples, rotates its end state into the window's
phase, and the row sums (xor butterfly). Those powers are not the oracle's
bits (the oracle runs one 1024-step chain per tone), so pass 0 decides a
window only where its top-2 margin clears the threshold t2e64 E P_max (E the
window's sum x^2) and leaves the rest to the exact chain. That is safe when

    |sqrt(P_pass0) - sigma(P_oracle)| <= rho_first sqrt(sum x^2)        (*)

on every window (sigma(P) = sign(P) sqrt|P|), rho_first the bound
audio-network_amd/csrc/error_model.cpp derives from pass 0's own double
operation sequence and the oracle's (demod_error_model; round 5: no measured
constant). This file restates pass 0's arithmetic in numpy
operation for operation (contraction is off in the kernel, so every product
and sum is rounded once, as here; the row sum in the kernel's butterfly
order), runs it on the adversarial signal families of tests/error_model.py
for tone plans from 0.3 bins to 511.7 bins, and asserts (*) against the
double oracle (oracle/fsk_oracle.c through oracle.goertzel), and that what
pass 0 decides is the oracle's symbol.
Test infrastructure: imports the oracle as the checker only.
"""
import math

import numpy as np
import pytest

import error_model as EM

FS = 48000.0
N = 1024
BIN = FS / N

# tone plans (Hz): the survey's, off-bin, and the band edges where the double
# recurrences are worst conditioned (the oracle's own error grows like
# 1 / sin^2 w there)
PLANS = {
    "fsk2": (1500.0, 3000.0),
    "fsk8": tuple(1500.0 + 375.0 * i for i in range(8)),
    "nonint8": tuple(1234.5 + 1111.1 * i for i in range(8)),
    "bins_1_2": (1 * BIN, 2 * BIN),
    "bin_0p3_3": (0.3 * BIN, 3 * BIN),
    "nyq_511_510": (511 * BIN, 510 * BIN),
    "nyq_511p7_500": (511.7 * BIN, 500 * BIN),
}


def rot64(freqs):
    """The host's [k][16] (A, B) segment rotations, A = e^{-i w (64 j + 63)}."""
    w = 2 * np.pi * np.asarray(freqs, np.float64)[:, None] / FS
    j = np.arange(16)[None, :]
    a, b = -w * (64 * j + 63), -w * (64 * j + 64)
    return np.cos(a), np.sin(a), np.cos(b), np.sin(b)


def butterfly_sum16(v):
    """The kernel's row sum: v += shfl_xor(v, m), m = 1, 2, 4, 8 (every lane
    ends with the same value; lane 0's is returned)."""
    idx = np.arange(16)
    for m in (1, 2, 4, 8):
        v = v + v[:, idx ^ m]
    return v[:, 0]


def pass0_powers(x, freqs, coef=None):
    """Pass 0's powers of W windows x[W][1024] (int16), operation for operation
    (coef: the chains' coefficients, default the oracle's 2 cos(2 pi f / fs))."""
    W = x.shape[0]
    xs = x.reshape(W, 16, 64).astype(np.float64)
    Ar, Ai, Br, Bi = rot64(freqs)
    P = np.empty((W, len(freqs)))
    for k, f in enumerate(freqs):
        c = 2.0 * math.cos(2.0 * math.pi * f / FS) if coef is None else coef[k]
        s1 = np.zeros((W, 16))
        s2 = np.zeros((W, 16))
        for i in range(64):
            s = xs[:, :, i] + c * s1
            s = s - s2
            s2, s1 = s1, s
        re = Ar[k] * s1
        im = Ai[k] * s1
        re = re - Br[k] * s2
        im = im - Bi[k] * s2
        re = butterfly_sum16(re)
        im = butterfly_sum16(im)
        P[:, k] = re * re + im * im
    return P


def _sigma(P):
    return np.sign(P) * np.sqrt(np.abs(P))


def _check(P, ref_sym, ref_P, x, m):
    """(*) on every window and tone; pass 0's decisions are the oracle's.
    Returns the worst error as a fraction of the bound."""
    xw = x.astype(np.float64)
    E = (xw * xw).sum(axis=1)
    bound = m["rho_first"] * np.sqrt(E)[:, None]
    d = np.abs(np.sqrt(P) - _sigma(ref_P))
    assert (d <= bound).all(), float((d / np.maximum(bound, 1e-300)).max())
    ok = bound[:, 0] > 0
    Ps = np.sort(P, axis=1)
    decided = (Ps[:, -1] > 0) & ((Ps[:, -1] - Ps[:, -2]) ** 2 >= m["t2e64"] * E * Ps[:, -1]) \
        & (16.0 * Ps[:, -1] >= m["t2e64"] * E)
    assert (np.argmax(P, axis=1)[decided] == ref_sym[decided]).all()
    return float((d[ok] / bound[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_pass0_error_model(A, O, plan):
    freqs = PLANS[plan]
    cfg = A.make_cfg(freqs=freqs, method=A.METHOD_GOERTZEL)
    m = A.error_model(cfg)
    info = A.plan_info(cfg)
    # K <= 2 on multiples of 8 bins (fsk2): the plain bank's pass 0 by the fold
    assert info["fold64"] == int(plan == "fsk2")
    assert m["rho_first"] > 0
    worst = (0.0, None)
    for fi, fam in enumerate(EM.FAMILIES):
        W = 384
        x = EM.family(fam, freqs, N, W, seed=100 + fi).reshape(W, N)
        ref_sym, ref_P = O.goertzel(x, freqs, N, fs=FS, threads=4)
        P = pass0_fold_powers(x, info, len(freqs)) if info["fold64"] else pass0_powers(x, freqs)
        r = _check(P, ref_sym, ref_P, x, m)
        worst = max(worst, (r, fam))
    print(f"\n{plan}: rho_first {m['rho_first']:.3g}, worst error {worst[0]:.3g} of it ({worst[1]})")


@pytest.mark.parametrize("plan", ["fsk2", "fsk8", "bins_1_2", "nyq_511_510"])
def test_fft_pass0_error_model(A, O, plan):
    """The FFT detector's first pass (rescue_fft.h rescue_fft_seg): the same
    segmented recurrence at its tone bins' frequencies, against the oracle's
    double radix-2 FFT powers of those bins (oracle.fft_demod)."""
    bins = [round(f * N / FS) for f in PLANS[plan]]
    freqs = tuple(b * FS / N for b in bins)
    cfg = A.make_cfg(freqs=PLANS[plan], method=A.METHOD_FFT)
    m = A.error_model(cfg)
    info = A.plan_info(cfg)
    # every bin a multiple of 8: pass 0 by the fold (plan.h fold64)
    assert info["fold64"] == int(all(b % 8 == 0 for b in bins))
    assert m["rho_first"] > 0
    worst = (0.0, None)
    for fi, fam in enumerate(EM.FAMILIES):
        W = 384
        x = EM.family(fam, freqs, N, W, seed=200 + fi).reshape(W, N)
        ref_sym, ref_P = O.fft_demod(x, PLANS[plan], N)
        if info["fold64"]:
            P = pass0_fold_powers(x, info, len(bins))
        else:
            P = pass0_powers(x, freqs, coef=[2.0 * math.cos(2.0 * math.pi * b / N) for b in bins])
        r = _check(P, ref_sym, ref_P, x, m)
        worst = max(worst, (r, fam))
    print(f"\nfft {plan}: rho_first {m['rho_first']:.3g}, worst error {worst[0]:.3g} of it ({worst[1]})")


# fold detector plans (every tone on a multiple of 8 bins; plan.h fold64):
# pass 0 by the fold (rescue_rows.h rescue_rows_fold0, rescue.hip
# rescue_seg_kernel), including the DC and Nyquist bins
FOLD_PLANS = {
    "fsk8": (tuple(1500.0 + 375.0 * i for i in range(8)), "AUTO"),
    "fold3_edges": ((8 * BIN, 16 * BIN, 504 * BIN), "AUTO"),
    "fold2_dc": ((0.0, 8 * BIN), "FOLDED"),
    "fold2_nyq": ((504 * BIN, 512 * BIN), "FOLDED"),
}


def pass0_fold_powers(x, info, K):
    """Pass 0 by the fold of W windows x[W][1024] (int16), operation for
    operation with the plan's own tables (demod_plan_info rot64: [k][16][4],
    then the chains' coefficients): lane j's folded samples xf[8j .. 8j+7]
    (exact integer sums over the 8 blocks of 128), an 8-step double chain per
    tone, the rotation, the 16-lane butterfly, the power."""
    W = x.shape[0]
    r = info["rot64"]
    rot = r[:64 * K].reshape(K, 16, 4)
    xf = x.astype(np.int64).reshape(W, 8, 128).sum(axis=1).reshape(W, 16, 8).astype(np.float64)
    P = np.empty((W, K))
    for k in range(K):
        c = r[64 * K + k]
        s1 = np.zeros((W, 16))
        s2 = np.zeros((W, 16))
        for i in range(8):
            s = xf[:, :, i] + c * s1
            s = s - s2
            s2, s1 = s1, s
        re = rot[k, :, 0] * s1
        im = rot[k, :, 1] * s1
        re = re - rot[k, :, 2] * s2
        im = im - rot[k, :, 3] * s2
        re = butterfly_sum16(re)
        im = butterfly_sum16(im)
        P[:, k] = re * re + im * im
    return P


@pytest.mark.parametrize("plan", sorted(FOLD_PLANS))
def test_fold_pass0_error_model(A, O, plan):
    freqs, meth = FOLD_PLANS[plan]
    cfg = A.make_cfg(freqs=freqs, method=getattr(A, "METHOD_" + meth))
    info = A.plan_info(cfg)
    assert info["method"] == A.METHOD_FOLDED and info["fold64"] == 1
    # the exact chains keep the oracle's coefficients after pass 0's
    K = len(freqs)
    assert np.array_equal(info["rot64"][65 * K:66 * K], info["rcoef"])
    m = A.error_model(cfg)
    assert m["rho_first"] > 0
    worst = (0.0, None)
    for fi, fam in enumerate(EM.FAMILIES):
        W = 384
        x = EM.family(fam, freqs, N, W, seed=300 + fi).reshape(W, N)
        ref_sym, ref_P = O.goertzel(x, freqs, N, fs=FS, threads=4)
        r = _check(pass0_fold_powers(x, info, K), ref_sym, ref_P, x, m)
        worst = max(worst, (r, fam))
    print(f"\nfold {plan}: rho_first {m['rho_first']:.3g}, worst error {worst[0]:.3g} of it ({worst[1]})")


# residue detector plans (integer bins, not all multiples of 8; plan.h fold64
# = 2): pass 0 by the residue fold (rescue.hip seg_residue_window), every
# residue class 0 .. 7 and the band edges
RESIDUE_PLANS = {
    "odd8": tuple((32 + 9 * i) * BIN for i in range(8)),        # residues 0, 1, ..., 7
    "edges4": (1 * BIN, 2 * BIN, 511 * BIN, 510 * BIN),         # residues 1, 2, 7, 6
    "k16": tuple((20 + 7 * i) * BIN for i in range(16)),
    "nyq_dc": (0.0, 4 * BIN, 508 * BIN, 512 * BIN),             # residues 0, 4, 4, 0 (real Y)
}
KC = 0.70710678118654752440


def pass0_residue_powers(x, info, K):
    """Pass 0 by the residue fold of W windows x[W][1024] (int16), operation
    for operation: lane j's samples x[128 m + 8 j + i], the exact integer
    butterflies a_m = x_m + x_{m+4}, d_m = x_m - x_{m+4}, Y_rho (odd rho: d0
    +- c u, +-d2 +- c v, each product and sum rounded once), the real and
    imaginary 8-step chains at the exact bin, the complex rotation, the
    16-lane butterfly, the power."""
    W = x.shape[0]
    r = info["rot64"]
    rot = r[:64 * K].reshape(K, 16, 4)
    xs = x.astype(np.int64).reshape(W, 8, 16, 8)               # [w][m][j][i]
    a = [xs[:, m] + xs[:, m + 4] for m in range(4)]            # [w][j][i], exact
    d = [xs[:, m] - xs[:, m + 4] for m in range(4)]
    P = np.empty((W, K))
    for k in range(K):
        c = r[64 * K + k]
        rho = int(r[66 * K + k])
        if rho in (0, 4):
            sg = 1 if rho == 0 else -1
            yr, yi = ((a[0] + a[2]) + sg * (a[1] + a[3])).astype(np.float64), None
        elif rho in (2, 6):
            sg = -1 if rho == 2 else 1
            yr = (a[0] - a[2]).astype(np.float64)
            yi = (sg * (a[1] - a[3])).astype(np.float64)
        else:
            cu = KC * (d[1] - d[3]).astype(np.float64)
            cv = KC * (d[1] + d[3]).astype(np.float64)
            d0 = d[0].astype(np.float64)
            d2 = ((-1 if rho in (1, 5) else 1) * d[2]).astype(np.float64)
            yr = d0 + cu if rho in (1, 7) else d0 - cu
            yi = d2 - cv if rho in (1, 3) else d2 + cv

        def chain(y):
            s1 = np.zeros((W, 16))
            s2 = np.zeros((W, 16))
            for i in range(8):
                s = y[:, :, i] + c * s1
                s = s - s2
                s2, s1 = s1, s
            return s1, s2
        a1, a2 = chain(yr)
        R = rot[k]
        if yi is None:
            re = R[:, 0] * a1
            im = R[:, 1] * a1
            re = re - R[:, 2] * a2
            im = im - R[:, 3] * a2
        else:
            b1, b2 = chain(yi)
            re = (R[:, 0] * a1 - R[:, 1] * b1) - (R[:, 2] * a2 - R[:, 3] * b2)
            im = (R[:, 0] * b1 + R[:, 1] * a1) - (R[:, 2] * b2 + R[:, 3] * a2)
        re = butterfly_sum16(re)
        im = butterfly_sum16(im)
        P[:, k] = re * re + im * im
    return P


@pytest.mark.parametrize("plan", sorted(RESIDUE_PLANS))
def test_residue_pass0_error_model(A, O, plan):
    freqs = RESIDUE_PLANS[plan]
    cfg = A.make_cfg(freqs=freqs, method=A.METHOD_RESIDUE)
    info = A.plan_info(cfg)
    assert info["method"] == A.METHOD_RESIDUE and info["fold64"] == 2
    K = len(freqs)
    bins = [round(f / BIN) for f in freqs]
    assert np.array_equal(info["rot64"][66 * K:67 * K], [b % 8 for b in bins])
    assert np.array_equal(info["rot64"][65 * K:66 * K], info["rcoef"])
    m = A.error_model(cfg)
    assert m["rho_first"] > 0
    worst = (0.0, None)
    for fi, fam in enumerate(EM.FAMILIES):
        W = 384
        x = EM.family(fam, freqs, N, W, seed=400 + fi).reshape(W, N)
        ref_sym, ref_P = O.goertzel(x, freqs, N, fs=FS, threads=4)
        r = _check(pass0_residue_powers(x, info, K), ref_sym, ref_P, x, m)
        worst = max(worst, (r, fam))
    print(f"\nresidue {plan}: rho_first {m['rho_first']:.3g}, worst error {worst[0]:.3g} of it ({worst[1]})")
