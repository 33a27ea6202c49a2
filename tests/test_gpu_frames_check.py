"""Checked frames on the GPU (frames_check.hip) against tests/frames_check_ref.py.

Kernel level: test-made hits, packed rows and results on the device, so no
detector runs. Every output buffer is poisoned and compared WHOLE with the
reference laid over the same poison: one comparison says that what must be
written is written, byte for byte, and that nothing else is. Validity is
always the reference's verdict on the same bytes, so a random row that happens
to pass a CRC is an OK row on both sides.

End to end: five planted frames (one corrupted, one holding a copy of the word
and a valid frame in its data) through the detector and demod_frames_checked,
and through the segmented scan and demod_frames_check_async.
"""
import numpy as np
import pytest

import fec_modes_ref as Z
import frames_check_ref as C
import frames_ref as F
import guards as G
from gpu_support import handle_fixture, phased, results_bytes, same, tones_375, torch  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPE_OF_R = {1: (1024, 1024), 4: (1024, 256), 64: (512, 8)}    # (n, hop) of a handle with R phases
RES_BYTES = F.RESULT_DTYPE.itemsize
LEAD = 4096          # guard bytes per side (a multiple of 8: the aligned outputs stay aligned)
POISON = 0xFF


# handle(R, K): one Demodulator per (R, K), closed with the module.
handle = handle_fixture(lambda A, Rn, K: phased(A, SHAPE_OF_R, Rn, tones_375(K)))


def row_symbols(B, bits):
    """A frame_symbols whose packed row is B bytes."""
    N = (B * 8) // bits
    assert (N * bits + 7) // 8 == B
    return N


def expected(hits, packed, n_written, L, Rn, bits, h, kind, poison=POISON):
    """The four outputs whole: the reference laid over poison."""
    n_groups, max_frames, B = packed.shape
    max_len = B - h - C.CRC_BYTES[kind]
    chk = np.full((n_groups, max_frames, 16), poison, np.uint8)
    kept = np.full((n_groups, max_frames, 4), poison, np.uint8)
    body = np.full((n_groups, max_frames, max_len), poison, np.uint8)
    summ = np.zeros(n_groups, C.SUMMARY_DTYPE)
    refs = C.check_groups(hits, packed, n_written, max_frames, L, Rn, Z.span_of(bits, h, kind, 0), None, h, kind)
    for g, (r_chk, r_kept, r_bodies, r_summ) in enumerate(refs):
        chk[g, :len(r_chk)] = r_chk.view(np.uint8).reshape(-1, 16)
        kept[g, :len(r_kept)] = r_kept.view(np.uint8).reshape(-1, 4)
        for r, data in enumerate(r_bodies):
            body[g, r, :len(data)] = np.frombuffer(data, np.uint8)
        summ[g] = r_summ
    return dict(check=chk, kept=kept, body=body, summary=summ.view(np.uint8).reshape(n_groups, 32)), refs


class Run:
    """One call on test-made inputs: every output poisoned (and, with guard,
    between poisoned guard bands)."""

    def __init__(self, torch, hits, packed, n_written, body=True, poison=POISON, guard=False):
        self.torch = torch
        self.n_groups, self.max_frames, self.B = packed.shape
        self.inputs = [np.ascontiguousarray(hits).view(np.uint8).reshape(-1), packed.reshape(-1),
                       results_bytes(n_written).reshape(-1)]
        self.d_in = [torch.from_numpy(a.copy()).cuda() for a in self.inputs]
        self.want_body, self.poison, self.guard = body, poison, guard
        self.checks = []

    def out(self, nbytes):
        torch = self.torch
        if nbytes == 0:
            return torch.empty(0, dtype=torch.uint8, device="cuda")
        if not self.guard:
            return torch.full((nbytes,), self.poison, dtype=torch.uint8, device="cuda")
        t, chk = G.guarded(torch, nbytes, torch.uint8, LEAD, LEAD, self.poison)
        self.checks.append(chk)
        return t

    def __call__(self, d, L, N, h, kind, stream=0):
        torch = self.torch
        rows = self.n_groups * self.max_frames
        max_len = self.B - h - C.CRC_BYTES[kind]
        o = dict(check=self.out(rows * 16), kept=self.out(rows * 4),
                 body=self.out(rows * max_len) if self.want_body else None,
                 summary=self.out(self.n_groups * 32))
        d.frames_check_async(self.d_in[0], self.d_in[1], self.d_in[2], self.n_groups, self.max_frames, L, N,
                             h, kind, o["check"], o["kept"].view(torch.int32), o["body"], o["summary"],
                             stream=stream)
        torch.cuda.synchronize()
        for chk in self.checks:
            chk(written=False)
        for t, a in zip(self.d_in, self.inputs):
            assert np.array_equal(t.cpu().numpy(), a), "an input was written to"
        shape = dict(check=(self.n_groups, self.max_frames, 16), kept=(self.n_groups, self.max_frames, 4),
                     body=(self.n_groups, self.max_frames, max_len), summary=(self.n_groups, 32))
        return {k: v.cpu().numpy().reshape(shape[k]) for k, v in o.items() if v is not None}


def frame_row(rng, length, B, h, kind):
    """A valid frame of `length` random data bytes, random bytes behind it."""
    row = rng.integers(0, 256, B).astype(np.uint8)
    f = C.encode(rng.integers(0, 256, length).astype(np.uint8).tobytes(), h, kind)
    row[:len(f)] = np.frombuffer(f, np.uint8)
    return row


def flip(row, lo, hi, rng):
    """The row with one bit flipped in bytes lo .. hi-1."""
    out = row.copy()
    out[int(rng.integers(lo, hi))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    return out


# ---- CRC shapes ------------------------------------------------------------------

def crc_rows(rng, B, h, kind):
    c = C.CRC_BYTES[kind]
    max_len = B - h - c
    top = min(max_len, 256 ** h - 1)          # the longest length the header can say
    lens = [0] + [n for n in (1, max_len) if 0 < n <= top] + rng.integers(0, top + 1, 6).tolist()
    rows = []
    for n in lens:
        good = frame_row(rng, n, B, h, kind)
        rows.append(good)
        if n:
            rows.append(flip(good, h, h + n, rng))           # data
        rows.append(flip(good, h + n, h + n + c, rng))       # CRC
        rows.append(flip(good, 0, h, rng))                   # length
    if max_len + 1 < 256 ** h:
        long_row = rng.integers(0, 256, B).astype(np.uint8)
        long_row[:h] = np.frombuffer((max_len + 1).to_bytes(h, "big"), np.uint8)
        rows.append(long_row)
    rows += list(rng.integers(0, 256, (6, B)).astype(np.uint8))
    return np.array(rows, np.uint8)


@pytest.mark.parametrize("kind", [C.CRC16, C.CRC32])
@pytest.mark.parametrize("h", [1, 2])
def test_crc_shapes(A, torch, handle, h, kind):
    """Rows of h + c, h + c + 1, 63, 64, 65, 130 and 300 bytes and the row whose
    max_len is 4096: lengths 0, 1 and max_len, random valid frames, each with a
    bit flipped in its data, its CRC and its length, max_len + 1, random rows."""
    d = handle(4, 2)
    c = C.CRC_BYTES[kind]
    statuses = set()
    for B in (h + c, h + c + 1, 63, 64, 65, 130, 300, h + c + 4096):
        rng = np.random.default_rng(1000 * B + 10 * h + kind)
        rows = crc_rows(rng, B, h, kind)
        nw, max_frames = len(rows), len(rows) + 3
        packed = rng.integers(0, 256, (1, max_frames, B)).astype(np.uint8)
        packed[0, :nw] = rows
        hits = np.zeros((1, max_frames), C.HIT_DTYPE)
        hits["window"] = np.arange(max_frames) * 10 ** 6          # nothing covers anything
        want, refs = expected(hits, packed, [nw], 24, 4, 1, h, kind)
        got = Run(torch, hits, packed, [nw])(d, 24, row_symbols(B, 1), h, kind)
        same(got, want, B)
        statuses |= set(refs[0][0]["status"].tolist())
        assert refs[0][0]["status"][0] == C.OK and refs[0][3]["n_kept"] == refs[0][3]["n_valid"] >= 1
    assert statuses == {C.OK, C.BAD_LENGTH, C.BAD_CRC}


# ---- select shapes ---------------------------------------------------------------

SELECT_L, SELECT_B, SELECT_H, SELECT_KIND = 24, 8, 1, C.CRC16     # max_len 5
EDGES = (64, 128, 256, 512, 1024)


def select_group(rng, nw, rows_total, Rn, bits):
    """rows_total rows (the first nw are the group's) with ascending windows:
    at every wave and chunk edge e the rows e-3 .. e+2 are kept, covered,
    invalid | kept, covered, invalid; a frame of max_len at row 752 covers rows
    753 .. 782 (across the chunk edge 768), alternately valid and invalid; the
    rest is drawn. Returns
    (windows, rows, the roles that were forced)."""
    B, h, kind, L = SELECT_B, SELECT_H, SELECT_KIND, SELECT_L
    max_len = B - h - C.CRC_BYTES[kind]
    forced = {}
    for e in EDGES:
        if e + 3 <= nw:
            forced.update({e - 3: "kept", e - 2: "covered", e - 1: "invalid",
                           e: "kept", e + 1: "covered", e + 2: "invalid"})
    if nw > 800:
        forced[752] = "long"
        forced.update({i: "covered" if i % 2 else "invalid" for i in range(753, 783)})
    windows = np.zeros(rows_total, np.uint64)
    rows = np.zeros((rows_total, B), np.uint8)
    w, reach = int(rng.integers(0, 3)) * Rn, 0
    for i in range(rows_total):
        role = forced.get(i) or ("kept", "covered", "invalid", "random")[int(rng.integers(0, 4))]
        length = max_len if role == "long" else int(rng.integers(0, max_len + 1))
        w += Rn
        if role in ("kept", "long"):
            w = max(w, reach) + Rn * int(rng.integers(0, 3))     # touching the frame before, or past it
        elif role == "covered" and reach <= w:
            role = "kept"
        if role == "random":
            rows[i] = rng.integers(0, 256, B)
            rows[i, 0] = rng.integers(0, max_len + 3)
        else:
            rows[i] = frame_row(rng, length, B, h, kind)
            if role == "invalid":
                rows[i] = flip(rows[i], h, h + length + C.CRC_BYTES[kind], rng)     # data or CRC
        windows[i] = w
        if C.check_row(rows[i], h, kind)[2] == C.OK:
            reach = max(reach, w + (L + C.frame_symbols(h + C.check_row(rows[i], h, kind)[0] + 2, bits)) * Rn)
    return windows, rows, forced


@pytest.mark.parametrize("K", [2, 5, 8, 16])
@pytest.mark.parametrize("Rn", [1, 4, 64])
def test_select_shapes(A, torch, handle, Rn, K):
    """Groups of 0, 1, 63, 64, 65, 255, 256, 257 and 1025 rows, one of
    max_frames rows and two whose stored n_written is above max_frames."""
    d = handle(Rn, K)
    bits = F.bits_per_symbol(K)
    max_frames = 1030
    counts = [0, 1, 63, 64, 65, 255, 256, 257, 1025, max_frames, max_frames + 7, 2 ** 64 - 1]
    rng = np.random.default_rng(100 * Rn + K)
    hits = np.zeros((len(counts), max_frames), C.HIT_DTYPE)
    packed = np.zeros((len(counts), max_frames, SELECT_B), np.uint8)
    forced = []
    for g, n in enumerate(counts):
        hits["window"][g], packed[g], roles = select_group(rng, min(n, max_frames), max_frames, Rn, bits)
        hits["errors"][g] = rng.integers(0, 3, max_frames)
        forced.append(roles)
    want, refs = expected(hits, packed, counts, SELECT_L, Rn, bits, SELECT_H, SELECT_KIND)
    # the fixture's condition, on the reference alone: the forced roles came out
    seen = 0
    for roles, (chk, kept, _, summ) in zip(forced, refs):
        for i, role in roles.items():
            ok, cov = chk["status"][i] == C.OK, chk["covered"][i] == 1
            assert (role == "invalid" and not ok) or (role in ("kept", "long") and ok and not cov) or \
                (role == "covered" and ok and cov), (i, role, chk[i])
            seen += 1
        assert summ["n_checked"] >= summ["n_valid"] >= summ["n_kept"]
        assert summ["n_kept"] == len(kept) and (np.diff(kept.astype(np.int64)) > 0).all()
    assert seen >= 200
    got = Run(torch, hits, packed, counts)(d, SELECT_L, row_symbols(SELECT_B, bits), SELECT_H, SELECT_KIND)
    same(got, want, (Rn, K))


# ---- groups ----------------------------------------------------------------------

@pytest.mark.parametrize("n_groups", [1, 3, 1024])
def test_groups(A, torch, handle, n_groups):
    """Differing row counts, empty groups included; and a group's outputs do
    not depend on its slot or its neighbours: the same content in another slot
    gives the same bytes."""
    Rn, K, bits = 4, 2, 1
    d = handle(Rn, K)
    max_frames = 70 if n_groups <= 3 else 20
    rng = np.random.default_rng(n_groups)
    counts = rng.integers(0, max_frames + 1, n_groups).tolist()
    counts[0] = max_frames - 1
    if n_groups > 1:
        counts[1], counts[-1] = 0, max_frames
    hits = np.zeros((n_groups, max_frames), C.HIT_DTYPE)
    packed = np.zeros((n_groups, max_frames, SELECT_B), np.uint8)
    for g in range(n_groups):
        hits["window"][g], packed[g], _ = select_group(rng, counts[g], max_frames, Rn, bits)
    want, refs = expected(hits, packed, counts, SELECT_L, Rn, bits, SELECT_H, SELECT_KIND)
    N = row_symbols(SELECT_B, bits)
    got = Run(torch, hits, packed, counts)(d, SELECT_L, N, SELECT_H, SELECT_KIND)
    same(got, want, n_groups)
    assert sum(int(r[3]["n_kept"]) for r in refs) > n_groups
    # group 0's content in the last slot of a call of another size, among other neighbours
    S2 = n_groups + 2
    order = [(g + 1) % n_groups for g in range(n_groups)] + [n_groups - 1, 0]
    got2 = Run(torch, hits[order], packed[order], [counts[g] for g in order])(
        d, SELECT_L, N, SELECT_H, SELECT_KIND)
    for k in got:
        assert np.array_equal(got2[k][S2 - 1], got[k][0]), k
        assert np.array_equal(got2[k][:n_groups], got[k][order[:n_groups]]), k


# ---- guards ----------------------------------------------------------------------

@pytest.mark.parametrize("body", [True, False])
@pytest.mark.parametrize("Rn,K,h,kind,B", [(4, 2, 1, C.CRC16, 8), (1, 16, 2, C.CRC32, 65), (64, 8, 2, C.CRC16, 9)])
def test_guards(A, torch, handle, Rn, K, h, kind, B, body):
    """Every output between poisoned guards, two poisons: the guards and every
    byte the contract does not list keep the poison, every listed byte is
    written (it equals the reference under both poisons), the inputs are
    unchanged. Without d_body the other three outputs are the same."""
    d = handle(Rn, K)
    bits = F.bits_per_symbol(K)
    rng = np.random.default_rng(B + Rn)
    counts, max_frames = [40, 0, 300], 300
    N = (B * 8 + bits - 1) // bits
    assert (N * bits + 7) // 8 == B
    hits = np.zeros((3, max_frames), C.HIT_DTYPE)
    packed = rng.integers(0, 256, (3, max_frames, B)).astype(np.uint8)
    max_len = B - h - C.CRC_BYTES[kind]
    for g in range(3):
        w = 0
        for i in range(max_frames):
            if rng.integers(0, 3):
                packed[g, i] = frame_row(rng, int(rng.integers(0, min(max_len, 255) + 1)), B, h, kind)
            w += Rn * int(rng.integers(1, 200))
            hits["window"][g, i] = w
    for poison in (0xFF, 0x5A):
        want, refs = expected(hits, packed, counts, 8, Rn, bits, h, kind, poison)
        got = Run(torch, hits, packed, counts, body=body, poison=poison, guard=True)(d, 8, N, h, kind)
        assert ("body" in got) == body
        same(got, want, poison)
        assert 0 < refs[2][3]["n_kept"] < refs[2][3]["n_valid"] < 300      # the fixture's condition


# ---- refusals --------------------------------------------------------------------

def test_refusals(A, torch, handle):
    """Every DEMOD_BAD_ARG case returns without a launch: the outputs stay poison."""
    lib = A.load_library()
    d = handle(4, 2)
    S, cap, N, L = 3, 16, 64, 8                     # B = 8
    rows = S * cap

    def poison(nbytes):
        return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    d_hits = torch.zeros(rows * 16 + 8, dtype=torch.uint8, device="cuda")
    d_packed = torch.zeros(rows * 8 + 8, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(S * RES_BYTES + 8, dtype=torch.uint8, device="cuda")
    d_check, d_kept, d_body, d_sum = poison(rows * 16 + 8), poison(rows * 4 + 8), poison(rows * 5), poison(S * 32 + 8)
    ph, pp, pr, pc, pk, pb, ps = (t.data_ptr() for t in (d_hits, d_packed, d_res, d_check, d_kept, d_body, d_sum))

    def call(h=d._h, hits=ph, packed=pp, res=pr, n_groups=S, max_frames=cap, sync_len=L, n=N, len_bytes=1,
             crc=A.DEMOD_CRC16_CCITT_FALSE, check=pc, kept=pk, body=pb, summ=ps):
        return lib.demod_frames_check_async(h, hits, packed, res, n_groups, max_frames, sync_len, n,
                                            len_bytes, crc, check, kept, body, summ, None)

    cases = dict([
        ("NULL handle", dict(h=None)),
        ("NULL d_hits", dict(hits=None)),
        ("NULL d_packed", dict(packed=None)),
        ("NULL d_results", dict(res=None)),
        ("NULL d_check", dict(check=None)),
        ("NULL d_kept", dict(kept=None)),
        ("NULL d_summary", dict(summ=None)),
        ("misaligned d_hits", dict(hits=ph + 4)),
        ("misaligned d_results", dict(res=pr + 4)),
        ("misaligned d_summary", dict(summ=ps + 4)),
        ("misaligned d_check", dict(check=pc + 2)),
        ("misaligned d_kept", dict(kept=pk + 2)),
        ("n_groups == 0", dict(n_groups=0)),
        ("n_groups > DEMOD_MAX_SEGMENTS", dict(n_groups=A.DEMOD_MAX_SEGMENTS + 1, max_frames=1)),
        ("n_groups * max_frames >= 2^31", dict(n_groups=2 ** 15, max_frames=2 ** 16)),
        ("max_frames >= 2^31", dict(n_groups=1, max_frames=2 ** 31)),
        ("max_frames == 0", dict(max_frames=0)),
        ("sync_len == 0", dict(sync_len=0)),
        ("sync_len > DEMOD_MAX_SYNC", dict(sync_len=A.DEMOD_MAX_SYNC + 1)),
        ("len_bytes 0", dict(len_bytes=0)),
        ("len_bytes 3", dict(len_bytes=3)),
        ("crc 0", dict(crc=0)),
        ("crc 3", dict(crc=3)),
        ("B < h + c", dict(n=16)),
        ("B < h + c, CRC-32", dict(n=40, len_bytes=2, crc=A.DEMOD_CRC32_MPEG2)),
        ("frame_symbols == 0", dict(n=0)),
        ("max_len > DEMOD_MAX_FRAME_PAYLOAD", dict(n=8 * (4096 + 4), n_groups=1, max_frames=1)),
        ("frame_symbols >= 2^31", dict(n=2 ** 31)),
    ])
    for what, kw in cases.items():
        assert call(**kw) == A.DEMOD_BAD_ARG, what
    others = [A.Demodulator(n=1024, hop=384, freqs=(1500.0, 3000.0)),
              A.Demodulator(n=1024, hop=8, freqs=(1500.0, 3000.0))]
    try:
        for dd, what in zip(others, ("n % hop != 0", "R > 64")):
            assert call(h=dd._h) == A.DEMOD_BAD_ARG, what
    finally:
        for dd in others:
            dd.close()
    # the Python mirror's own checks (before any pointer reaches the library)
    full = dict(d_hits=d_hits, d_packed=d_packed, d_results=d_res, d_check=d_check, d_kept=d_kept[:rows * 4],
                d_body=d_body, d_summary=d_sum)
    for kw in (dict(d_hits=d_hits[:rows * 16 - 1]), dict(d_packed=d_packed[:rows * 8 - 1]),
               dict(d_results=d_res[:S * RES_BYTES - 1]), dict(d_check=d_check[:rows * 16 - 1]),
               dict(d_kept=d_kept[:rows * 4 - 4]), dict(d_kept=d_kept[:rows * 4].view(torch.int32).to(torch.int64)),
               dict(d_body=d_body[:rows * 5 - 1]), dict(d_summary=d_sum[:S * 32 - 1]), dict(d_check=None),
               dict(d_packed=d_packed.cpu()), dict(d_summary=d_sum.to(torch.int16))):
        a = dict(full)
        a.update(kw)
        if a["d_kept"].dtype == torch.uint8:
            a["d_kept"] = a["d_kept"].view(torch.int32)
        with pytest.raises(A.DemodError) as e:
            d.frames_check_async(a["d_hits"], a["d_packed"], a["d_results"], S, cap, L, N, 1,
                                 A.DEMOD_CRC16_CCITT_FALSE, a["d_check"], a["d_kept"], a["d_body"], a["d_summary"])
        assert e.value.code == A.DEMOD_BAD_ARG
    torch.cuda.synchronize()
    for t in (d_check, d_kept, d_body, d_sum):
        assert bool((t == 0xFF).all()), "a refused call wrote"
    # and the same call, legal, runs: three empty groups; the longest legal row too
    assert call() == A.DEMOD_OK
    torch.cuda.synchronize()
    assert not d_sum[:S * 32].cpu().numpy().any()
    assert bool((d_check == 0xFF).all()) and bool((d_kept == 0xFF).all()) and bool((d_body == 0xFF).all())
    big = torch.zeros(4102, dtype=torch.uint8, device="cuda")
    assert call(n=8 * 4102, n_groups=1, max_frames=1, packed=big.data_ptr(), len_bytes=2,
                crc=A.DEMOD_CRC32_MPEG2, body=None) == A.DEMOD_OK
    torch.cuda.synchronize()


# ---- a scan in front: determinism, capture and replay -----------------------------

SCAN_R, SCAN_K, SCAN_L, SCAN_N, SCAN_CAP = 4, 2, 24, 160, 24      # B = 20, h = 2, CRC-16: max_len 16


def scan_content(seed, n_frames, W=70001):
    """sym[W], P[W][2] and the word: n_frames frames on phase 1 among random
    symbols, every third with the word and a valid empty frame inside its data
    (a covered hit), every fourth with a flipped symbol."""
    rng = np.random.default_rng(seed)
    Rn, K, L, N = SCAN_R, SCAN_K, SCAN_L, SCAN_N
    sym = rng.integers(0, K, W).astype(np.uint8)
    P = np.repeat(rng.integers(1, 1024, (W, 1)).astype(np.float32), K, axis=1)
    P[1::Rn] *= np.float32(8.0)
    word = np.random.default_rng(5).integers(0, K, L).astype(np.uint8)
    w = 1 + 40 * Rn
    for f in range(n_frames):
        data = rng.integers(0, 256, int(rng.integers(0, 17))).astype(np.uint8).tobytes()
        if f % 3 == 1:          # the word and a valid empty frame inside this one's data: a covered hit
            data = data[:2].ljust(2, b"x") + np.packbits(word).tobytes() + C.encode(b"", 2, C.CRC16) + data[:3]
        row = C.payload_row(C.encode(data, 2, C.CRC16), N, 1, rng)
        if f % 4 == 3:
            row[16 + int(rng.integers(0, 8 * len(data) + 1))] ^= 1      # data or CRC
        sym[w:w + L * Rn:Rn] = word
        sym[w + L * Rn:w + (L + N) * Rn:Rn] = row
        w += (2 * (L + N) + 30 + int(rng.integers(0, 50))) * Rn
    assert w < W
    return sym, np.ascontiguousarray(P), word


def scan_reference(sym, P, word):
    hits, _, packed, res = F.frames(sym, P, SCAN_R, word, 0, SCAN_N, max_frames=SCAN_CAP)
    nw = res["n_written"]
    h2 = np.zeros((1, SCAN_CAP), C.HIT_DTYPE)
    p2 = np.zeros((1, SCAN_CAP, 20), np.uint8)
    h2[0, :nw], p2[0, :nw] = hits, packed
    want, refs = expected(h2, p2, [nw], SCAN_L, SCAN_R, 1, 2, C.CRC16)
    return res, want, refs[0]


class ScanBuffers:
    def __init__(self, A, torch, d, W):
        self.A, self.torch, self.d, self.W = A, torch, d, W
        u8 = dict(dtype=torch.uint8, device="cuda")
        self.d_sym = torch.zeros(W, **u8)
        self.d_P = torch.zeros((W, SCAN_K), dtype=torch.float32, device="cuda")
        self.d_work = torch.empty(A.frames_workspace_size(d.cfg, W), **u8)
        self.d_hits, self.d_packed = torch.empty(SCAN_CAP * 16, **u8), torch.empty(SCAN_CAP * 20, **u8)
        self.d_res = torch.empty(RES_BYTES, **u8)
        self.outs = dict(check=torch.empty(SCAN_CAP * 16, **u8), kept=torch.empty(SCAN_CAP * 4, **u8),
                         body=torch.empty(SCAN_CAP * 16, **u8), summary=torch.empty(32, **u8))

    def load(self, sym, P):
        self.d_sym.copy_(self.torch.from_numpy(sym))
        self.d_P.copy_(self.torch.from_numpy(P))

    def poison(self):
        for t in (self.d_hits, self.d_packed, self.d_res, *self.outs.values()):
            t.fill_(POISON)

    def step(self, word, stream=0):
        o = self.outs
        self.d.frames_async(self.d_sym, self.d_P, self.W, word, 0, SCAN_N, self.d_hits, None, self.d_packed,
                            SCAN_CAP, self.d_res, self.d_work, stream=stream)
        self.d.frames_check_async(self.d_hits, self.d_packed, self.d_res, 1, SCAN_CAP, SCAN_L, SCAN_N, 2,
                                  C.CRC16, o["check"], o["kept"].view(self.torch.int32), o["body"],
                                  o["summary"], stream=stream)

    def results(self):
        self.torch.cuda.synchronize()
        shape = dict(check=(1, SCAN_CAP, 16), kept=(1, SCAN_CAP, 4), body=(1, SCAN_CAP, 16), summary=(1, 32))
        return {k: v.cpu().numpy().reshape(shape[k]) for k, v in self.outs.items()}


def test_determinism_and_second_stream(A, torch, handle):
    """Two runs, and a run on a second stream with buffers of its own, give
    byte-identical outputs: the reference's."""
    d = handle(SCAN_R, SCAN_K)
    sym, P, word = scan_content(3, 14)
    res, want, ref = scan_reference(sym, P, word)
    assert res["phase"] == 1 and res["n_hits"] >= 14 and 0 < ref[3]["n_kept"] < ref[3]["n_valid"] < res["n_hits"]
    runs = []
    a, b = ScanBuffers(A, torch, d, len(sym)), ScanBuffers(A, torch, d, len(sym))
    for buf in (a, b):
        buf.load(sym, P)
        buf.poison()
    a.step(word)
    runs.append(a.results())
    a.poison()
    a.step(word)
    runs.append(a.results())
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b.step(word, stream=side.cuda_stream)
    runs.append(b.results())
    for r in runs:
        same(r, want)


def test_capture_and_replay(A, torch, handle):
    """demod_frames_async + demod_frames_check_async in one graph on a side
    stream, replayed after the symbols were rewritten in place: each replay's
    bytes are the reference's for that content."""
    d = handle(SCAN_R, SCAN_K)
    contents = [scan_content(3, 14), scan_content(4, 6)]
    refs = [scan_reference(*c) for c in contents]
    assert [int(r[2][3]["n_kept"]) for r in refs][0] != [int(r[2][3]["n_kept"]) for r in refs][1]
    buf = ScanBuffers(A, torch, d, len(contents[0][0]))
    word = contents[0][2]
    assert np.array_equal(word, contents[1][2])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        buf.load(*contents[0][:2])
        buf.poison()
        buf.step(word, stream=side.cuda_stream)          # an eager call of the shape first
        side.synchronize()
    same(buf.results(), refs[0][1], "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        buf.step(word, stream=torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        for (sym, P, _), (_, want, _) in zip(contents, refs):
            buf.load(sym, P)
            buf.poison()
            torch.cuda.synchronize()
            g.replay()
            same(buf.results(), want, rep)


# ---- end to end --------------------------------------------------------------------

E2E_L, E2E_LENS = 24, (5, 0, 12, 40, 9)
E2E_CORRUPT, E2E_HOST = 2, 3                   # frame 2: a flipped data symbol; frame 3 holds the copy


def e2e_stream(freqs, h=2, kind=C.CRC16, n=1024, hop=256, sigma=400.0, amplitude=8000.0, seed=77):
    """Five frames of different lengths as FSK with a random phase per symbol
    plus Gaussian noise, symbol boundaries on window starts. Returns (x int16,
    word, N, windows of the planted words, datas, the window of the copy)."""
    rng = np.random.default_rng(seed + len(freqs))
    K, Rn = len(freqs), n // hop
    bits = F.bits_per_symbol(K)
    word = rng.integers(0, K, E2E_L).astype(np.uint8)
    N = C.frame_symbols(h + max(E2E_LENS) + C.CRC_BYTES[kind], bits) + 5
    datas = [rng.integers(0, 256, m).astype(np.uint8).tobytes() for m in E2E_LENS]
    # the copy: the word's symbols and a valid empty frame as bytes, symbol-aligned in the host frame's data
    o = next(o for o in range(8) if ((h + o) * 8) % bits == 0)
    copy = F.pack(word[None, :], bits)[0].tobytes() + C.encode(b"", h, kind)
    assert (E2E_L * bits) % 8 == 0 and o + len(copy) <= E2E_LENS[E2E_HOST]
    host = bytearray(datas[E2E_HOST])
    host[o:o + len(copy)] = copy
    datas[E2E_HOST] = bytes(host)
    seq, at = [rng.integers(0, K, 9).astype(np.uint8)], []
    for f, data in enumerate(datas):
        at.append(sum(len(s) for s in seq))
        row = C.payload_row(C.encode(data, h, kind), N, bits, rng, K)
        if f == E2E_CORRUPT:
            j = C.frame_symbols(h, bits) + 1                     # a data symbol
            row[j] = (row[j] + 1) % K
        seq += [word, row, rng.integers(0, K, 8 + 3 * f).astype(np.uint8)]
    seq.append(rng.integers(0, K, 4).astype(np.uint8))
    truth = np.concatenate(seq)
    t = np.arange(n)
    ph = rng.uniform(0, 2 * np.pi, truth.size)
    w = 2 * np.pi * np.asarray(freqs, np.float64)[truth] / 48000.0
    v = amplitude * np.sin(w[:, None] * t[None, :] + ph[:, None]) + rng.normal(0.0, sigma, (truth.size, n))
    x = np.clip(np.round(v), -32768, 32767).astype(np.int16).reshape(-1)
    windows = [a * Rn for a in at]
    copy_window = windows[E2E_HOST] + (E2E_L + ((h + o) * 8) // bits) * Rn
    return np.ascontiguousarray(x), word, N, windows, datas, copy_window


@pytest.mark.parametrize("name", ["FSK2", "FSK8"])
def test_end_to_end(A, torch, name):
    """Detector, frame scan and check in one call: the four good frames come
    back with their windows, lengths and bytes; the corrupted one and the copy
    inside a frame's data do not. The summary is the reference's on the
    device's own scan outputs. Then the same batch as two segments through
    demod_frames_segments_async + demod_frames_check_async."""
    freqs = getattr(F, name)
    h, kind = 2, C.CRC16
    bits, Rn = F.bits_per_symbol(len(freqs)), 4
    x, word, N, windows, datas, copy_window = e2e_stream(freqs)
    B = (N * bits + 7) // 8
    max_len = B - h - C.CRC_BYTES[kind]
    good = [f for f in range(len(datas)) if f != E2E_CORRUPT]
    with A.Demodulator(n=1024, hop=256, freqs=freqs) as d:
        s_hits, _, s_packed, s_res = d.frames(x, word, max_errors=1, frame_symbols=N)
        nw = s_res["n_written"]
        assert s_res["phase"] == 0 and s_res["n_hits"] == nw
        assert set(windows) | {copy_window} <= set(s_hits["window"].tolist())     # the scan lists them all
        chk, kept, bodies, summ = C.check_group(s_hits["window"], s_packed, E2E_L, Rn, Z.span_of(bits, h, kind, 0),
                                                None, h, kind)
        for pcm in (x, torch.from_numpy(x).cuda()):
            hits, lengths, body, res, summary = d.frames_checked(pcm, word, max_errors=1, frame_symbols=N,
                                                                len_bytes=h, crc=kind)
            assert len(hits) == summary["n_kept"] == len(good)
            assert hits["window"].tolist() == [windows[f] for f in good]
            assert lengths.tolist() == [len(datas[f]) for f in good]
            assert body == [datas[f] for f in good] == bodies
            assert summary == dict(n_checked=nw, n_valid=int(summ["n_valid"]), n_kept=len(good), reserved=0)
            assert summary["n_valid"] == len(good) + 1          # the copy is valid, and covered
            assert hits.tobytes() == s_hits[kept].tobytes()
            assert {f: res[f] for f in res if f != "metric"} == {f: s_res[f] for f in s_res if f != "metric"}
        i_copy = s_hits["window"].tolist().index(copy_window)
        assert chk[i_copy].tolist() == (0, C.crc(kind, bytes(h)), C.OK, 1)
        assert chk["status"][s_hits["window"].tolist().index(windows[E2E_CORRUPT])] == C.BAD_CRC
        # a short max_frames cuts the scan, and says so
        hits, lengths, body, res, summary = d.frames_checked(x, word, max_errors=1, frame_symbols=N,
                                                            len_bytes=h, crc=kind, max_frames=2, body=False)
        assert res["n_hits"] == nw > res["n_written"] == 2 == summary["n_checked"] and body is None
        assert hits["window"].tolist() == [w for w in s_hits["window"][:2].tolist() if w in windows[:2]]
        # two segments, cut in the gap before frame 3
        W = (len(x) - 1024) // 256 + 1
        cut = windows[3] - 4 * Rn
        first, count = [0, cut], [cut, W - cut]
        seg = d.frames_segments(x, first, count, word, max_errors=1, frame_symbols=N, payload=False)
        cap = 8
        u8 = dict(dtype=torch.uint8, device="cuda")
        d_pcm = torch.from_numpy(x).cuda()
        d_sym, d_mag = torch.empty(W, **u8), torch.empty(W * d.k, dtype=torch.float32, device="cuda")
        d_first = torch.from_numpy(np.array(first, np.int64)).cuda()
        d_count = torch.from_numpy(np.array(count, np.int32)).cuda()
        d_hits, d_packed, d_results = torch.full((2 * cap * 16,), POISON, **u8), torch.full((2 * cap * B,), POISON, **u8), \
            torch.empty(2 * RES_BYTES, **u8)
        d_work = torch.empty(A.frames_segments_workspace_size(d.cfg, 2, W), **u8)
        outs = dict(check=torch.full((2 * cap * 16,), POISON, **u8), kept=torch.full((2 * cap * 4,), POISON, **u8),
                    body=torch.full((2 * cap * max_len,), POISON, **u8), summary=torch.full((64,), POISON, **u8))
        d.batch_async(d_pcm, W, d_sym, d_mag)
        d.frames_segments_async(d_sym, d_mag, W, d_first, d_count, 2, word, 1, N, d_hits, None, d_packed, cap,
                                d_results, d_work)
        d.frames_check_async(d_hits, d_packed, d_results, 2, cap, E2E_L, N, h, kind, outs["check"],
                             outs["kept"].view(torch.int32), outs["body"], outs["summary"])
        torch.cuda.synchronize()
        h2 = d_hits.cpu().numpy().view(C.HIT_DTYPE).reshape(2, cap)
        p2 = d_packed.cpu().numpy().reshape(2, cap, B)
        n_written = [r[3]["n_written"] for r in seg]
        for s in range(2):                 # the device rows are the synchronous call's
            assert h2[s, :n_written[s]].tobytes() == seg[s][0].tobytes()
            assert np.array_equal(p2[s, :n_written[s]], seg[s][2])
        want, refs = expected(h2, p2, n_written, E2E_L, Rn, bits, h, kind)
        shape = dict(check=(2, cap, 16), kept=(2, cap, 4), body=(2, cap, max_len), summary=(2, 32))
        same({k: v.cpu().numpy().reshape(shape[k]) for k, v in outs.items()}, want, "segments")
        kept_windows = [int(h2[s, i]["window"]) + first[s] for s in range(2) for i in refs[s][1]]
        assert kept_windows == [windows[f] for f in good]
        assert [b for s in range(2) for b in refs[s][2]] == [datas[f] for f in good]
