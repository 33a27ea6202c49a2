"""The stages behind the decode in every coded mode (include/demod.h "punctured
and interleaved"): the coded check's `covered` selection (frames_check.hip)
under the mode's span and at the mode's row width, and the one-shot
demod_frames_coded, against tests/fec_modes_ref.py.

Kernel level as test_coded_check of tests/test_gpu_frames_fec.py: test-made
hits, rows and results on the device, so no detector, no scan and no decode
run. Every output is poisoned and compared WHOLE with the reference laid over
the same poison; the inputs are compared byte for byte after the call. Spans,
row shapes and lengths on the expected side are counted by fec_modes_ref; no
library function gives them.

A check that took another span passes unless a hit lies between the two: the
cases place one there for each span a per-mode slip would give (alt_spans),
and tests/test_fec_stages_cpu.py asserts on the reference alone that each of
them changes `covered`.

End to end: five coded frames as 2-FSK and 8-FSK PCM in every mapped mode,
payload symbols of three of them on a wrong tone, through demod_frames_coded
from a host array and from a device pointer, against rx_ref.scan_check
on the device detector's own outputs.
"""
import functools

import numpy as np
import pytest

import fec_modes_ref as Z
import frames_check_ref as C
import frames_fec_ref as X
import frames_ref as F
import rx_ref as RX
import test_gpu_frames_fec as TF
from gpu_support import handle_fixture, phased, tones_375, torch  # noqa: F401

pytestmark = pytest.mark.gpu

MAX_LEN = 40         # rows that hold every edge length of fec_modes_ref.edge_lengths
L0 = 8               # the word's symbols in the kernel-level tests (it is never read)
POISONS = (0xFF, 0x5A)
# (K, R) x (h, CRC) of the single-group cases, and the one case at 16 tones with R 64
CHECK_SHAPES = [(K, Rn, h, kind) for K, Rn in ((2, 1), (8, 4)) for h, kind in ((1, C.CRC16), (2, C.CRC32))]
CHECK_CASES = [(fec,) + s for fec in Z.MODES for s in CHECK_SHAPES] + [(0x51, 16, 64, 1, C.CRC16)]
GROUPS_SHAPE = dict(K=8, Rn=4, h=1, kind=C.CRC16, n_groups=65, max_frames=5)


# handle(R, K): one Demodulator per (R, K), closed with the module.
handle = handle_fixture(lambda A, Rn, K: phased(A, TF.SHAPE_OF_R, Rn, tones_375(K)))


# ---- the spans a per-mode slip would give ------------------------------------------------

def alt_spans(length, bits, h, kind, fec):
    """The symbols a frame would span under (a) the rate-1/2 count 2 T, (b) the
    mode's kept bits without the block rounding, (c) the block rounding without
    the puncturing; (b) and (c) where the mode has the flag they leave out."""
    T = X.steps(length, h, kind)
    out = {"a": -(-2 * T // bits)}
    if fec & Z.INTERLEAVE:
        out["b"] = -(-Z.kept_bits(fec, T) // bits)
        if fec & 0x30:
            out["c"] = -(-(-(-2 * T // Z.BLOCK) * Z.BLOCK) // bits)
    return out


def covered_under(windows, rows, L, Rn, h, kind, span):
    """`covered` of one group's rows with span(length) symbols behind the word."""
    out, reach = [], 0
    for w, row in zip(windows, rows):
        length, _, status = C.check_row(row, h, kind)
        cov = 0
        if status == C.OK:
            cov = int(reach > int(w))
            reach = max(reach, int(w) + (L + span(length)) * Rn)
        out.append(cov)
    return np.array(out, np.uint8)


def case_lengths(bits, h, kind, fec):
    """(N, Bd, max_len, the lengths): rows that hold MAX_LEN bytes, the mode's
    edge lengths up to MAX_LEN, 30 (where the spans of 0x41 and 0x51 differ,
    which coincide at 40) and the rows' own max_len."""
    N = Z.symbols_for(MAX_LEN, bits, h, kind, fec)
    St, Bd, max_len = Z.row_shape(N, bits, h, kind, fec)
    return N, Bd, max_len, sorted(set(Z.edge_lengths(MAX_LEN, h, kind, fec)) | {30, max_len})


def frame_bytes(rng, n, h, kind):
    return np.frombuffer(C.encode(rng.integers(0, 256, n).astype(np.uint8).tobytes(), h, kind), np.uint8)


@functools.lru_cache(maxsize=None)
def check_case(fec, K, Rn, h, kind):
    """One group of pairs (A, B): A starts past every span of what lies before
    it, B relative to A: touching A's end under the mode's span (kept), one
    window inside (covered), past it, and between the mode's span and each
    alternative span that differs from it at A's length. Then a row that stores
    max_len + 1 and a CRC-invalid row, each with a frame where it would reach.
    Returns a dict: hits [1][mf], rows [1][mf][Bd], nw, N, the gap of each row."""
    bits = F.bits_per_symbol(K)
    N, Bd, max_len, lens = case_lengths(bits, h, kind, fec)
    rng = np.random.default_rng(fec * 1000 + K * 10 + Rn + h)

    def span(n):
        return Z.span(n, bits, h, kind, fec)

    def far(n):
        return max([span(n)] + list(alt_spans(n, bits, h, kind, fec).values()))
    windows, frames, gaps = [], [], []
    w, other = 5, 0
    for n in lens:
        own = span(n)
        offsets = {"touch": (L0 + own) * Rn, "inside": (L0 + own) * Rn - 1, "past": (L0 + own + 7) * Rn}
        for name, alt in alt_spans(n, bits, h, kind, fec).items():
            lo, hi = min(own, alt), max(own, alt)
            if (hi - lo) * Rn >= 2:
                offsets["between " + name] = (L0 + lo) * Rn + (hi - lo) * Rn // 2
        for gap, off in offsets.items():
            m = lens[other % len(lens)]
            other += 1
            windows += [w, w + off]
            frames += [frame_bytes(rng, n, h, kind), frame_bytes(rng, m, h, kind)]
            gaps += ["first", gap]
            w = max(w + (L0 + far(n)) * Rn, w + off + (L0 + far(m)) * Rn) + 3 + other % 5
    long_row = rng.integers(0, 256, Bd).astype(np.uint8)
    long_row[:h] = np.frombuffer((max_len + 1).to_bytes(h, "big"), np.uint8)
    bad_crc = frame_bytes(rng, 20, h, kind).copy()
    bad_crc[h] ^= 1
    for row, name in ((long_row, "long"), (bad_crc, "invalid")):
        windows += [w, w + (L0 + 5) * Rn]                 # inside every span of a row that was valid
        frames += [row, frame_bytes(rng, 7, h, kind)]
        gaps += [name, "behind " + name]
        w += 2 * (L0 + far(max_len)) * Rn
    nw = len(windows)
    hits = np.zeros((1, nw + 2), C.HIT_DTYPE)
    hits["window"][0, :nw] = windows
    hits["errors"] = rng.integers(0, 3, hits.shape)
    rows = rng.integers(0, 256, (1, nw + 2, Bd)).astype(np.uint8)
    for i, f in enumerate(frames):
        rows[0, i, :len(f)] = f
    return dict(hits=hits, rows=rows, counts=[nw], N=N, gaps=gaps, bits=bits, lens=lens)


@functools.lru_cache(maxsize=None)
def groups_case(fec):
    """65 groups of up to 5 rows at the mode's width: frames of drawn lengths
    placed touching, inside, past or between the mode's span and the rate-1/2
    one behind the row before; every fifth row invalid. Group 1 is empty, group
    2 stores n_written = max_frames + 7, groups 0 and 64 hold the same rows."""
    g = GROUPS_SHAPE
    K, Rn, h, kind, n_groups, mf = (g[k] for k in ("K", "Rn", "h", "kind", "n_groups", "max_frames"))
    bits = F.bits_per_symbol(K)
    N, Bd, max_len, lens = case_lengths(bits, h, kind, fec)
    rng = np.random.default_rng(65 + fec)
    hits = np.zeros((n_groups, mf), C.HIT_DTYPE)
    rows = rng.integers(0, 256, (n_groups, mf, Bd)).astype(np.uint8)
    counts = [int(v) for v in rng.integers(1, mf + 1, n_groups)]
    counts[0], counts[1], counts[2], counts[n_groups - 1] = mf, 0, mf + 7, mf
    for s in range(n_groups):
        w = int(rng.integers(0, 9))
        for i in range(mf):
            n = lens[int(rng.integers(0, len(lens)))]
            f = frame_bytes(rng, n, h, kind).copy()
            if (s + i) % 5 == 4:
                f[h + len(f) % 3] ^= 0x10
            rows[s, i, :len(f)] = f
            hits["window"][s, i] = w
            own, half = Z.span(n, bits, h, kind, fec), X.coded_symbols(n, h, kind, bits)
            off = [(L0 + own) * Rn, (L0 + own) * Rn - 1, (L0 + own + 3) * Rn,
                   (L0 + min(own, half)) * Rn + abs(own - half) * Rn // 2][int(rng.integers(0, 4))]
            w += off
    hits["errors"] = rng.integers(0, 3, hits.shape)
    hits[n_groups - 1], rows[n_groups - 1] = hits[0], rows[0]
    return dict(hits=hits, rows=rows, counts=counts, N=N, bits=bits, lens=lens)


def expected(case, Rn, h, kind, fec, poison):
    return TF.coded_expected(case["hits"], case["rows"], case["counts"], L0, Rn, case["bits"], h, kind, poison, fec)


def run_check(torch, d, case, Rn, h, kind, fec):
    """demod_frames_check_coded_async on the case under two poisons: check,
    kept, body and summary whole equal the reference with the mode's span; the
    inputs are unwritten. Returns the reference's per-group results."""
    hits, rows = case["hits"], case["rows"]
    n_groups, mf, Bd = rows.shape
    max_len = Bd - h - C.CRC_BYTES[kind]
    inputs = [hits.view(np.uint8).reshape(-1), rows.reshape(-1), TF.results_bytes(case["counts"]).reshape(-1)]
    d_in = [torch.from_numpy(a.copy()).cuda() for a in inputs]
    u8 = dict(dtype=torch.uint8, device="cuda")
    shape = dict(check=(n_groups, mf, 16), kept=(n_groups, mf, 4), body=(n_groups, mf, max_len), summary=(n_groups, 32))
    for poison in POISONS:
        want, refs = expected(case, Rn, h, kind, fec, poison)
        o = {k: torch.full((int(np.prod(s)),), poison, **u8) for k, s in shape.items()}
        d.frames_check_coded_async(d_in[0], d_in[1], d_in[2], n_groups, mf, L0, case["N"], h, kind, o["check"],
                                   o["kept"].view(torch.int32), o["body"], o["summary"], fec=fec)
        torch.cuda.synchronize()
        TF.same({k: v.cpu().numpy().reshape(shape[k]) for k, v in o.items()}, want, (hex(fec), poison))
    for t, a in zip(d_in, inputs):
        assert t.cpu().numpy().tobytes() == a.tobytes(), "an input was written to"
    return refs


# ---- the coded check ----------------------------------------------------------------------

@pytest.mark.parametrize("fec,K,Rn,h,kind", CHECK_CASES)
def test_coded_check_modes(A, torch, handle, fec, K, Rn, h, kind):
    """Every mode (0x01 the control) at 2 tones with R 1 and 8 tones with R 4, h
    1 with CRC-16 and h 2 with CRC-32, and 0x51 at 16 tones with R 64: rows at
    the mode's Bd, the edge lengths, 30 and max_len; a stored length of max_len
    + 1 is BAD_LENGTH and a CRC-invalid row covers nothing. What the placement
    proves is asserted by tests/test_fec_stages_cpu.py without a GPU."""
    case = check_case(fec, K, Rn, h, kind)
    refs = run_check(torch, handle(Rn, K), case, Rn, h, kind, fec)
    chk = refs[0][0]
    gaps = case["gaps"]
    assert chk["status"][gaps.index("long")] == C.BAD_LENGTH and chk["status"][gaps.index("invalid")] == C.BAD_CRC
    assert not chk["covered"][gaps.index("behind long")] and not chk["covered"][gaps.index("behind invalid")]


@pytest.mark.parametrize("fec", Z.NEW_MODES)
def test_coded_check_groups(A, torch, handle, fec):
    """65 groups of up to 5 rows, an empty group and one whose stored n_written
    is above max_frames: each group's rows are read at the mode's width (47 or
    63 bytes with the interleaver, 43 without), and the same rows in groups 0
    and 64 give the same bytes."""
    g = GROUPS_SHAPE
    case = groups_case(fec)
    refs = run_check(torch, handle(g["Rn"], g["K"]), case, g["Rn"], g["h"], g["kind"], fec)
    assert refs[1][3]["n_checked"] == 0 and refs[2][3]["n_checked"] == g["max_frames"]
    assert refs[0][0].tobytes() == refs[64][0].tobytes() and refs[0][2] == refs[64][2]


# ---- end to end: demod_frames_coded ----------------------------------------------------------

E2E_L, E2E_LENS, E2E_HIT, E2E_H, E2E_KIND = TF.E2E_L, TF.E2E_LENS, TF.E2E_HIT, 2, C.CRC16
# Wrong-tone symbols per marked frame: three, as test_end_to_end of tests/test_gpu_frames_fec.py, except in
# mode 0x21 at 8 tones: a wrong tone inverts up to three neighbouring air bits, rate 3/4 without the
# interleaver has free distance 5, and with three wrong symbols the reference alone loses a frame for
# some draws of the powers (tests/test_fec_stages_cpu.py decodes these very rows under several). With two
# it recovers all five under every draw; every other mode does with three.
E2E_WRONG = {(0x21, 8): 2}


def air_symbols(air, N, bits, rng):
    """N row symbols: the air bits `air`, random bits behind them."""
    b = np.concatenate([air, rng.integers(0, 2, max(0, N * bits - air.size)).astype(np.uint8)])[:N * bits]
    return (b.reshape(N, bits) << np.arange(bits - 1, -1, -1, dtype=np.uint8)).sum(axis=1).astype(np.uint8)


def e2e_symbols(K, fec, wrong=None, seed=91):
    """Five frames of the mode (fec_modes_ref.encode) among random symbols; in
    three of them `wrong` well-separated payload symbols sit on a wrong tone.
    Returns (the symbol sequence, word, N, the words' symbol indices, datas,
    the sent payload rows, wrong)."""
    rng = np.random.default_rng(seed + K + fec)
    bits, h, kind = F.bits_per_symbol(K), E2E_H, E2E_KIND
    wrong = E2E_WRONG.get((fec, K), 3) if wrong is None else wrong
    word = rng.integers(0, K, E2E_L).astype(np.uint8)
    N = Z.symbols_for(max(E2E_LENS), bits, h, kind, fec) + 3
    datas = [rng.integers(0, 256, m).astype(np.uint8).tobytes() for m in E2E_LENS]
    seq, at, sent = [rng.integers(0, K, 9).astype(np.uint8)], [], []
    for f, data in enumerate(datas):
        at.append(sum(len(s) for s in seq))
        air = np.unpackbits(np.frombuffer(Z.encode(data, h, kind, fec), np.uint8))
        air = air[:Z.air_bits(fec, X.steps(len(data), h, kind))]
        row = air_symbols(air, N, bits, rng)
        sent.append(row.copy())
        if f in E2E_HIT:
            Sc = Z.span(len(data), bits, h, kind, fec)
            for j in (Sc // 6, Sc // 2, (5 * Sc) // 6)[:wrong]:
                row[j] = (row[j] + 1 + int(rng.integers(0, K - 1))) % K
        seq += [word, row, rng.integers(0, K, 8 + 3 * f).astype(np.uint8)]
    seq.append(rng.integers(0, K, 4).astype(np.uint8))
    return np.concatenate(seq), word, N, at, datas, sent, wrong


def e2e_pcm(freqs, truth, seed, n=1024, sigma=400.0, amplitude=8000.0):
    """The symbols as FSK with a random phase per symbol plus Gaussian noise
    (the signal and the noise level of test_end_to_end)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    ph = rng.uniform(0, 2 * np.pi, truth.size)
    w = 2 * np.pi * np.asarray(freqs, np.float64)[truth] / 48000.0
    x = np.empty((truth.size, n), np.int16)
    for a in range(0, truth.size, 512):                  # in slices: the whole signal in double is large
        v = amplitude * np.sin(w[a:a + 512, None] * t[None, :] + ph[a:a + 512, None]) + \
            rng.normal(0.0, sigma, (len(w[a:a + 512]), n))
        x[a:a + 512] = np.clip(np.round(v), -32768, 32767)
    return np.ascontiguousarray(x.reshape(-1))


@pytest.mark.parametrize("name", ["FSK2", "FSK8"])
@pytest.mark.parametrize("fec", Z.NEW_MODES)
def test_frames_coded_modes(A, torch, fec, name):
    """demod_frames_coded in every mapped mode, n 1024, hop 256: bodies,
    lengths, kept hits and summary equal rx_ref.scan_check (scan, the
    mode's decode, the coded check with the mode's span) on the device
    detector's own (sym, P); all five bodies come back although the hard
    decisions of three rows differ from what was sent. From a host array and
    from a device pointer."""
    freqs = getattr(F, name)
    h, kind, n, hop = E2E_H, E2E_KIND, 1024, 256
    K, bits, Rn = len(freqs), F.bits_per_symbol(len(freqs)), n // hop
    truth, word, N, at, datas, sent, wrong = e2e_symbols(K, fec)
    windows = [a * Rn for a in at]
    x = e2e_pcm(freqs, truth, 7 + K + fec)
    u8 = dict(dtype=torch.uint8, device="cuda")
    with A.Demodulator(n=n, hop=hop, freqs=freqs) as d:
        W = (len(x) - n) // hop + 1
        d_pcm = torch.from_numpy(x).cuda()
        d_sym, d_mag = torch.empty(W, **u8), torch.empty(W * K, dtype=torch.float32, device="cuda")
        d.batch_async(d_pcm, W, d_sym, d_mag)
        torch.cuda.synchronize()
        sym, P = d_sym.cpu().numpy(), d_mag.cpu().numpy().reshape(W, K)
        for f, w0 in enumerate(windows):             # the hard decisions: wrong where a wrong tone was sent
            Sc = Z.span(len(datas[f]), bits, h, kind, fec)
            hard = sym[w0 + (E2E_L + np.arange(Sc)) * Rn]
            assert int((hard != sent[f][:Sc]).sum()) == (wrong if f in E2E_HIT else 0), f
        r_hits, r_chk, r_kept, r_bodies, r_summ, r_res = RX.scan_check(sym, P, Rn, word, 1, N, h, kind, fec)
        nw = r_res["n_written"]
        assert r_bodies == datas and [int(r_hits["window"][i]) for i in r_kept] == windows   # the reference alone
        assert r_res["phase"] == 0 and nw == len(r_hits)
        for pcm in (x, d_pcm):
            hits, lengths, body, res, summary = d.frames_coded(pcm, word, max_errors=1, frame_symbols=N,
                                                              len_bytes=h, crc=kind, fec=fec)
            assert body == r_bodies and lengths.tolist() == [len(b) for b in r_bodies]
            assert hits.tobytes() == r_hits[r_kept].tobytes()
            assert summary == dict(n_checked=nw, n_valid=int(r_summ["n_valid"]), n_kept=len(r_kept), reserved=0)
            assert {f: res[f] for f in res if f != "metric"} == {f: r_res[f] for f in r_res if f != "metric"}
