"""The receiver on the GPU (frames_carry.hip, demod_rx.cpp) against
tests/rx_ref.py.

Stage level: demod_rx_advance_async on hand-made rings and demod_rx_collect_async
on hand-made check outputs, no detector and no scan. Every output is poisoned
and compared WHOLE with the reference laid over the same poison, between guard
bands (tests/guards.py): one comparison says that what must be written is
written, byte for byte, and that nothing else is.

Handle level, from PCM: the frames demod_rx_push returns over all pushes equal
the kept frames of demod_frames_checked (demod_frames_coded) on each stream's
whole recording, whatever the packet sizes; overflow, cut, reset and refusals.
"""
import ctypes

import numpy as np
import pytest

import frames_check_ref as C
import frames_ref as F
import guards as G
import link_ref as LR
import rx_ref as X
from gpu_support import handle_fixture, same, torch  # noqa: F401

pytestmark = pytest.mark.gpu

LEAD = 4096                      # guard bytes per side (a multiple of 8: aligned outputs stay aligned)
POISONS = (0xFF, 0x5A)
F32_POISONS = (G.F32_POISON, 0x5A5A5A5A)
N, HOP = 1024, 256
R = N // HOP
H, KIND, L_WORD = 1, C.CRC16, 16


def tones(K):
    return tuple(1500.0 + 375.0 * i for i in range(K))


# handle(K): one Demodulator (n 1024, hop 256) per K, closed with the module.
handle = handle_fixture(lambda A, K: A.Demodulator(n=N, hop=HOP, freqs=tones(K)))


class Outs:
    """Guarded, poisoned device outputs of one call."""

    def __init__(self, torch, poison, f32_poison):
        self.torch, self.poison, self.f32_poison, self.checks = torch, poison, f32_poison, []

    def u8(self, nbytes, init=None):
        t, chk = G.guarded(self.torch, max(nbytes, 8), self.torch.uint8, LEAD, LEAD, self.poison)
        self.checks.append(chk)
        t = t[:nbytes]
        if init is not None:
            t.copy_(self.torch.from_numpy(np.ascontiguousarray(init).view(np.uint8).reshape(-1)))
        return t

    def f32(self, numel):
        t, chk = G.guarded(self.torch, numel, self.torch.float32, LEAD, LEAD, self.f32_poison)
        self.checks.append(chk)
        return t

    def guards_intact(self):
        self.torch.cuda.synchronize()
        for chk in self.checks:
            chk(written=False)


# ---- advance ---------------------------------------------------------------------------

def advance_case(S, Cw, K, seed):
    """States, rings and a new batch that meet every clamp: keep in {0, 1, fill
    - 1, fill, fill + 5}, new counts in {0, 1, C - kept, C - kept + 1, C + 7}, a
    stored fill above C, a first past the batch and a count that runs past it."""
    rng = np.random.default_rng(seed)
    state = np.zeros(S, X.STATE_DTYPE)
    state["base"] = rng.integers(0, 2 ** 40, S)
    state["hold"], state["dropped"], state["cut_hits"] = rng.integers(0, 2 ** 40, (3, S))
    fill = rng.integers(0, Cw + 1, S)
    fill[::7] = Cw
    fill[3::11] = 0
    state["fill"] = fill
    keep_of = [lambda f: 0, lambda f: 1, lambda f: max(f - 1, 0), lambda f: f, lambda f: f + 5]
    state["keep"] = [keep_of[s % 5](int(fill[s])) for s in range(S)]
    if S > 2:
        state["fill"][2] = Cw + 9              # stored above C: clamped
    kept = np.minimum(state["fill"], Cw).astype(np.int64)
    kept -= np.minimum(state["keep"], kept)
    count_of = [lambda k: 0, lambda k: 1, lambda k: Cw - k, lambda k: Cw - k + 1, lambda k: Cw + 7]
    count = np.array([count_of[(s // 5 + s) % 5](int(kept[s])) for s in range(S)], np.int64)
    first = np.concatenate([[0], np.cumsum(count + (np.arange(S) % 3))[:-1]]).astype(np.int64) + 2
    W = int(first[-1] + count[-1]) + 4
    if S > 4:
        first[4] = W + 10                      # past the batch: no new windows
    if S > 1:
        count[S - 1] += 50                     # runs past the batch: clamped to its end
    ring_sym = rng.integers(0, K, (S, Cw)).astype(np.uint8)
    ring_mag = rng.integers(0, 2 ** 31 - 1, (S, Cw, K)).astype(np.int32)       # any bits: they are moved
    new_sym = rng.integers(0, K, W).astype(np.uint8)
    new_mag = rng.integers(0, 2 ** 31 - 1, (W, K)).astype(np.int32)
    return state, ring_sym, ring_mag, new_sym, new_mag, first.astype(np.uint64), count.astype(np.uint32)


@pytest.mark.parametrize("K", [2, 16])
@pytest.mark.parametrize("Cw", [96, 1000])
@pytest.mark.parametrize("S", [1, 3, 64, 65, 1025])
def test_advance(A, torch, handle, S, Cw, K):
    d = handle(K)
    state, ring_sym, ring_mag, new_sym, new_mag, first, count = advance_case(S, Cw, K, 1000 * S + Cw + K)
    d_in = [torch.from_numpy(a).cuda() for a in (ring_sym.reshape(-1), ring_mag.reshape(-1), new_sym,
                                                 new_mag.reshape(-1), first.view(np.int64), count.view(np.int32))]
    outs = []
    for poison, fp in zip(POISONS, F32_POISONS):
        o = Outs(torch, poison, fp)
        d_state = o.u8(S * 40, state)
        d_sym, d_mag = o.u8(S * Cw), o.f32(S * Cw * K)
        d_first, d_count = o.u8(S * 8), o.u8(S * 4)
        d.rx_advance_async(d_state, d_in[0], d_in[1].view(torch.float32), d_in[2], d_in[3].view(torch.float32),
                           len(new_sym), d_in[4], d_in[5], S, Cw, d_sym, d_mag, d_first.view(torch.int64),
                           d_count.view(torch.int32))
        o.guards_intact()
        w_state, w_sym, w_mag, w_first, w_count = X.advance(
            state, ring_sym, ring_mag, new_sym, new_mag, first, count, np.full((S, Cw), poison, np.uint8),
            np.full((S, Cw, K), fp, np.int32), np.frombuffer(bytes([poison]) * (8 * S), np.uint64),
            np.frombuffer(bytes([poison]) * (4 * S), np.uint32))
        same(d_state.cpu().numpy(), w_state.view(np.uint8), "state")
        same(d_sym.cpu().numpy(), w_sym, "ring symbols")
        same(d_mag.view(torch.int32).cpu().numpy(), w_mag, "ring powers")
        same(d_first.cpu().numpy(), w_first.view(np.uint8), "first")
        same(d_count.cpu().numpy(), w_count.view(np.uint8), "count")
        outs.append((w_state, w_count))
    for t, a in zip(d_in, (ring_sym, ring_mag, new_sym, new_mag, first.view(np.int64), count.view(np.int32))):
        same(t.cpu().numpy(), a, "an input was written to")
    w_state, w_count = outs[0]
    assert (w_state["keep"] == 0).all() and (w_state["fill"] == w_count).all() and w_count.max() == Cw
    if S >= 64:
        assert (w_state["dropped"] > state["dropped"]).any() and (w_count == 0).any()


# ---- collect ---------------------------------------------------------------------------

MODE_LEN = 40                    # the mapped modes' rows hold frames of 40 bytes: 43 bytes wide, 47 or 63 interleaved
COLLECT_MODE_CASES = [(1, 5, 2), (65, 130, 2), (1025, 4, 2), (65, 130, 8)]       # (S, mf, K)


def collect_seed(S, mf, K, fec):
    return 77 * S + mf + fec + K


def collect_case(S, mf, K, fec, seed, mode_len=None):
    """Hand-made outputs of a scan and a check for S groups of up to mf rows.
    mode_len: rows of the smallest N that holds frames of that many bytes in
    mode fec (the mode's N, max_len and span)."""
    rng = np.random.default_rng(seed)
    bits = F.bits_per_symbol(K)
    h, kind = (2, C.CRC16) if fec else (1, C.CRC32)
    if mode_len is not None:
        Nsym = X.row_symbols(h, kind, fec, bits, mode_len)
    else:
        Nsym = 400 // bits if fec else X.row_symbols(h, kind, 0, bits, 7)
    max_len = X.sizes(K, R, S, L_WORD, Nsym, h, kind, fec, mf, 10 ** 6)["max_len"]
    state = np.zeros(S, X.STATE_DTYPE)
    state["base"] = rng.integers(0, 2 ** 40, S)
    state["dropped"], state["cut_hits"] = rng.integers(0, 2 ** 30, (2, S))
    state["fill"] = rng.integers(0, 3000, S)
    state["keep"] = rng.integers(0, 2 ** 31, S)
    hits = np.zeros((S, mf), C.HIT_DTYPE)
    hits["window"] = np.sort(rng.integers(0, 2900, (S, mf)), axis=1)
    hits["errors"] = rng.integers(0, 4, (S, mf))
    check = np.zeros((S, mf), C.CHECK_DTYPE)
    check["length"] = rng.choice([0, 1, max_len, max_len, 3, max_len + 9], (S, mf))
    check["crc"] = rng.integers(0, 2 ** 32, (S, mf))
    check["status"] = rng.choice([C.OK, C.OK, C.BAD_CRC, C.BAD_LENGTH], (S, mf))
    check["covered"] = rng.integers(0, 2, (S, mf))
    if mode_len is not None:      # stream 0 (hold 0, mf rows) emits a row whose stored length is above max_len
        check["length"][0, 0], check["status"][0, 0], check["covered"][0, 0] = max_len + 9, C.OK, 0
    res = np.zeros(S, X.RESULT_DTYPE)
    nw = rng.integers(0, mf + 1, S)
    nw[::5] = mf
    res["n_written"] = np.where(np.arange(S) % 9 == 4, mf + 3 + rng.integers(0, 2 ** 40, S), nw)   # stored above
    res["n_hits"] = res["n_written"] + rng.choice([0, 0, 1, 7], S)
    res["n_hits"][1::13] = 0                                                  # below n_written: no cut
    res["tail_window"] = np.where(rng.integers(0, 2, S) == 1, -1, rng.integers(0, 3300, S))
    res["phases"], res["phase"] = R, rng.integers(0, R, S)
    kept = rng.integers(0, mf + 3, (S, mf)).astype(np.uint32)                 # an entry >= mf is skipped
    summ = np.zeros(S, C.SUMMARY_DTYPE)
    for s in range(S):
        n = min(int(nw[s]), mf)
        ok = np.flatnonzero((check["status"][s, :n] == C.OK) & (check["covered"][s, :n] == 0))
        kept[s, :len(ok)] = ok
        summ["n_kept"][s] = len(ok) if s % 7 != 3 else mf + 1 + s             # stored above: what lies there counts
        summ["n_checked"][s], summ["n_valid"][s] = n, int((check["status"][s, :n] == C.OK).sum())
    summ["n_checked"][::17] = 2 ** 50
    # hold below, inside and above each group's rows
    mid = state["base"] + hits["window"][:, mf // 2]
    state["hold"] = np.select([np.arange(S) % 3 == 0, np.arange(S) % 3 == 1], [np.zeros(S, np.uint64), mid],
                              state["base"] + np.uint64(10 ** 6))
    body = rng.integers(0, 256, (S, mf, max_len)).astype(np.uint8)
    if S >= 3:      # the same group in another slot
        for a in (state, hits, check, res, kept, summ, body):
            a[S - 1] = a[0]
    return dict(state=state, hits=hits, res=res, check=check, kept=kept, body=body, summ=summ, h=h, kind=kind,
                N=Nsym, max_len=max_len, bits=bits)


def collect_reference(c, fec, poison=0xFF):
    """rx_ref.collect of a case over poisoned outputs: (state, frames, bodies, summary)."""
    S, mf = c["hits"].shape
    rows = S * mf
    return X.collect(c["state"], c["hits"], c["res"], c["check"], c["kept"], c["body"], c["summ"], L_WORD, R,
                     c["bits"], c["h"], c["kind"], fec, np.frombuffer(bytes([poison]) * (rows * 32), X.FRAME_DTYPE),
                     np.full(rows * c["max_len"], poison, np.uint8))


@pytest.mark.parametrize("fec", [0, 1])
@pytest.mark.parametrize("S,mf", [(1, 5), (63, 5), (64, 1), (65, 130), (1025, 4), (20000, 3)])
def test_collect(A, torch, handle, S, mf, fec):
    K = 2
    run_collect(A, torch, handle(K), collect_case(S, mf, K, fec, 77 * S + mf + fec), S, mf, fec)


@pytest.mark.parametrize("S,mf,K", COLLECT_MODE_CASES)
@pytest.mark.parametrize("fec", [0x11, 0x21, 0x41, 0x51, 0x61])
def test_collect_modes(A, torch, handle, fec, S, mf, K):
    """The same in the five mapped modes, with the mode's N, max_len and span:
    hold comes from the mode's span and a stored length above max_len is
    clamped at the mode's max_len. tests/test_fec_stages_cpu.py asserts on the
    reference alone that hold differs from the rate-1/2 one and that a clamped
    record is emitted."""
    run_collect(A, torch, handle(K), collect_case(S, mf, K, fec, collect_seed(S, mf, K, fec), MODE_LEN), S, mf, fec)


def run_collect(A, torch, d, c, S, mf, fec):
    """State, summary, records and bytes whole over two poisons, the guards
    intact, the inputs unwritten."""
    ins = [c["hits"], c["res"], c["check"], c["kept"], c["body"], c["summ"]]
    d_in = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda() for a in ins]
    rows, max_len = S * mf, c["max_len"]
    work_bytes = A.rx_collect_workspace_size(d.cfg, S)
    got = []
    for poison, fp in zip(POISONS, F32_POISONS):
        o = Outs(torch, poison, fp)
        d_state = o.u8(S * 40, c["state"])
        d_frames, d_bodies, d_summary = o.u8(rows * 32), o.u8(rows * max_len), o.u8(32)
        d_work = o.u8(work_bytes)
        d.rx_collect_async(d_state, d_in[0], d_in[1], d_in[2], d_in[3].view(torch.int32), d_in[4], d_in[5], S, mf,
                           L_WORD, c["N"], c["h"], c["kind"], fec, d_frames, d_bodies, d_summary, d_work)
        o.guards_intact()
        w_state, w_frames, w_bodies, w_summary = collect_reference(c, fec, poison)
        same(d_state.cpu().numpy(), w_state.view(np.uint8), "state")
        same(d_summary.cpu().numpy(), w_summary.reshape(1).view(np.uint8), "summary")
        same(d_frames.cpu().numpy(), w_frames.view(np.uint8), "records")
        same(d_bodies.cpu().numpy(), w_bodies, "bytes")
        got.append((w_frames, w_summary, w_state))
    for t, a in zip(d_in, ins):
        same(t.cpu().numpy(), np.ascontiguousarray(a).view(np.uint8), "an input was written to")
    frames, summary, w_state = got[0]
    n = int(summary["n_frames"])
    assert n > 0 or S == 1
    fr = frames[:n]
    assert (np.diff(fr["stream"].astype(np.int64)) >= 0).all()
    lens = fr["length"].astype(np.int64)
    assert fr["body"].astype(np.int64).tolist() == (np.cumsum(lens) - lens).tolist()
    assert (fr["length"] <= max_len).all() and int(summary["n_bytes"]) == int(fr["length"].sum())
    if S >= 3:      # the same group in another slot: the same records apart from stream and body
        a, b = fr[fr["stream"] == 0], fr[fr["stream"] == S - 1]
        for f in ("length", "window", "errors", "reserved"):
            assert a[f].tolist() == b[f].tolist()
        for f in ("hold", "keep", "cut_hits"):
            assert w_state[f][0] == w_state[f][S - 1]
    if S >= 63:
        assert (w_state["hold"] > c["state"]["hold"]).any() and (w_state["hold"] == c["state"]["hold"]).any()
        assert (w_state["cut_hits"] > c["state"]["cut_hits"]).any()


def test_stage_refusals(A, torch, handle):
    """What the two async entries refuse, in C, before any launch."""
    d = handle(2)
    lib, S, Cw, mf, Nsym = A.load_library(), 2, 96, 4, 64

    def z(n, dtype=torch.uint8):
        return torch.zeros(n, dtype=dtype, device="cuda")

    st, sym_a, sym_b = z(S * 40 + 8), z(S * Cw), z(S * Cw)
    mag_a, mag_b, new_sym, new_mag = z(S * Cw * 2 + 1, torch.float32), z(S * Cw * 2, torch.float32), z(16), \
        z(32, torch.float32)
    tab8, tab4, first, count = z(S + 1, torch.int64), z(S + 1, torch.int32), z(S, torch.int64), z(S, torch.int32)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def adv(**kw):
        a = dict(st=p(st), si=p(sym_a), mi=p(mag_a), ns=p(new_sym), nm=p(new_mag), W=16, nf=p(tab8), nc=p(tab4),
                 S=S, C=Cw, so=p(sym_b), mo=p(mag_b), f=p(first), c=p(count))
        a.update(kw)
        return lib.demod_rx_advance_async(d._h, a["st"], a["si"], a["mi"], a["ns"], a["nm"], a["W"], a["nf"],
                                          a["nc"], a["S"], a["C"], a["so"], a["mo"], a["f"], a["c"], None)

    assert adv() == A.DEMOD_OK
    for kw in (dict(st=None), dict(si=None), dict(mi=None), dict(ns=None), dict(nm=None), dict(nf=None),
               dict(nc=None), dict(so=None), dict(mo=None), dict(f=None), dict(c=None),
               dict(so=p(sym_a)), dict(mo=p(mag_a)), dict(S=0), dict(S=A.DEMOD_MAX_SEGMENTS + 1), dict(C=0),
               dict(S=2 ** 16, C=2 ** 15), dict(W=2 ** 31), dict(st=p(st, 4)), dict(nf=p(tab8, 4)),
               dict(f=p(first, 4)), dict(nc=p(tab4, 2)), dict(c=p(count, 2)), dict(mi=p(mag_a, 2))):
        assert adv(**kw) == A.DEMOD_BAD_ARG, kw
    rows = S * mf
    hits, res, chk, kept, body, summ = z(rows * 16 + 8), z(S * 560), z(rows * 16), z(rows, torch.int32), \
        z(rows * 5), z(S * 32)
    frames, bodies, summary, work = z(rows * 32 + 8), z(rows * 5), z(32 + 8), z(64)
    need = A.rx_collect_workspace_size(d.cfg, S)

    def col(**kw):
        a = dict(st=p(st), hits=p(hits), res=p(res), chk=p(chk), kept=p(kept), body=p(body), summ=p(summ), S=S,
                 mf=mf, L=8, N=Nsym, h=1, crc=C.CRC16, fec=0, fr=p(frames), bo=p(bodies), su=p(summary),
                 work=p(work), wb=need)
        a.update(kw)
        return lib.demod_rx_collect_async(d._h, a["st"], a["hits"], a["res"], a["chk"], a["kept"], a["body"],
                                          a["summ"], a["S"], a["mf"], a["L"], a["N"], a["h"], a["crc"], a["fec"],
                                          a["fr"], a["bo"], a["su"], a["work"], a["wb"], None)

    assert col() == A.DEMOD_OK
    for kw in (dict(st=None), dict(hits=None), dict(res=None), dict(chk=None), dict(kept=None), dict(body=None),
               dict(summ=None), dict(fr=None), dict(bo=None), dict(su=None), dict(work=None), dict(wb=need - 1),
               dict(S=0), dict(S=A.DEMOD_MAX_SEGMENTS + 1), dict(mf=0), dict(S=2 ** 15, mf=2 ** 16), dict(L=0),
               dict(L=65), dict(h=0), dict(h=3), dict(crc=0), dict(crc=3), dict(fec=2), dict(fec=1), dict(N=16),
               dict(st=p(st, 4)), dict(hits=p(hits, 4)), dict(fr=p(frames, 4)), dict(su=p(summary, 4)),
               dict(work=p(work, 4)), dict(chk=p(chk, 2)), dict(kept=p(kept, 2))):
        assert col(**kw) == A.DEMOD_BAD_ARG, kw
    torch.cuda.synchronize()


# ---- the handle, from PCM ----------------------------------------------------------------

MAX_LEN = 3


def rx_setup(A, K, fec, max_frames=8, ring=None, n_frames=5, seed=0):
    """A recording of n_frames frames as FSK and the receiver's configuration."""
    rng = np.random.default_rng(4000 + 10 * K + fec + seed)
    bits = F.bits_per_symbol(K)
    word = rng.integers(0, K, L_WORD).astype(np.uint8)
    Nsym = X.row_symbols(H, KIND, fec, bits, MAX_LEN)
    items = [6]
    for f in range(n_frames):
        items += [rng.integers(0, 256, int(rng.integers(0, MAX_LEN + 1))).astype(np.uint8).tobytes(), 3 + 2 * f]
    symbols, planted = X.stream_symbols(items + [Nsym + 4], K, word, H, KIND, fec, rng)
    pcm = X.synth_pcm(tones(K), symbols, N, 99 + K + fec + seed)
    W = (len(pcm) - N) // HOP + 1
    rxcfg = A.make_rx_cfg(word, 0, Nsym, H, KIND, fec, max_frames, ring or W + 64)
    return pcm, word, Nsym, rxcfg, [d for _, d in planted]


def one_shot(d, pcm, word, Nsym, fec):
    """[(window, errors, body)] of demod_frames_checked / demod_frames_coded."""
    if fec:
        hits, lengths, bodies, _, _ = d.frames_coded(pcm, word, 0, Nsym, H, KIND, fec=fec)
    else:
        hits, lengths, bodies, _, _ = d.frames_checked(pcm, word, 0, Nsym, H, KIND)
    return [(int(hh["window"]), int(hh["errors"]), b) for hh, b in zip(hits, bodies)]


def packets_of(total, scheme, seed=0):
    if scheme == "single":
        return [total]
    if scheme == "packets":
        return [2880] * (total // 2880) + ([total % 2880] if total % 2880 else [])
    rng = np.random.default_rng(seed)
    out, left = [0, 100, 997], total - 1097
    while left > 0:
        p = int(min(left, rng.choice([0, 100, 997, 2880, 5000, 9000])))
        out.append(p)
        left -= p
    return out


def run_streams(rx, recs, sizes, ch=1):
    """Pushes stream s's recording recs[s] in packets of sizes[s][i] frames
    (streams that ran out push nothing). Returns per stream [(window, errors,
    body)] in output order, and checks each push's list for its order."""
    S = len(recs)
    at, out = [0] * S, [[] for _ in range(S)]
    for i in range(max(len(z) for z in sizes)):
        pk = []
        for s in range(S):
            n = sizes[s][i] if i < len(sizes[s]) else 0
            pk.append(recs[s][at[s] * ch:(at[s] + n) * ch] if n else None)
            at[s] += n
        fr, bodies, summ = rx.push(pk)
        assert summ["n_frames"] == len(fr) and (np.diff(fr["stream"].astype(np.int64)) >= 0).all()
        assert fr["body"].tolist() == np.cumsum([0] + [len(b) for b in bodies])[:-1].tolist()
        assert (fr["reserved"] == 0).all() and [int(x) for x in fr["length"]] == [len(b) for b in bodies]
        for f, b in zip(fr, bodies):
            out[int(f["stream"])].append((int(f["window"]), int(f["errors"]), b))
    assert all(at[s] * ch == len(recs[s]) for s in range(S))
    return out


@pytest.mark.parametrize("fec", [0, 1])
@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("S", [1, 3, 65])
def test_push_gives_the_one_shot_frames(A, torch, handle, S, K, fec):
    """Five frames per stream, each stream delayed by its own number of samples:
    2880-frame packets, ragged packets (0, 100 and 997 frames among them) and one
    single push all return each stream's one-shot frames under its own index."""
    push_against_one_shot(A, handle(K), S, K, fec)


@pytest.mark.parametrize("fec", [0x21, 0x51, 0x61])
@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("S", [1, 3])
def test_push_gives_the_one_shot_frames_modes(A, torch, handle, S, K, fec):
    """The same in modes 0x21, 0x51 and 0x61: with tests/test_gpu_fec_modes.py's
    link every flag (rate 2/3, rate 3/4, interleaved) reaches a receiver at 1
    and at 3 bits a symbol, where a 256-bit block ends inside a symbol."""
    push_against_one_shot(A, handle(K), S, K, fec)


def push_against_one_shot(A, d, S, K, fec):
    pcm, word, Nsym, rxcfg, datas = rx_setup(A, K, fec)
    rng = np.random.default_rng(S)
    delays = [0 if S == 1 else HOP * ((3 * s) % 7) + 20 * (s % 5) for s in range(S)]
    recs = [np.concatenate([rng.integers(-300, 301, dl).astype(np.int16), pcm]) for dl in delays]
    want = {}
    for s, dl in enumerate(delays):
        if dl not in want:
            want[dl] = one_shot(d, recs[s], word, Nsym, fec)
            assert [b for _, _, b in want[dl]] == datas, "the fixture's frames all check out"
    rxcfg.ring_windows = (len(pcm) + max(delays)) // HOP + 64
    for scheme in ("packets", "ragged", "single"):
        with A.Receiver(S, rxcfg, n=N, hop=HOP, freqs=tones(K)) as rx:
            got = run_streams(rx, recs, [packets_of(len(r), scheme, 11 * s) for s, r in enumerate(recs)])
            for s, dl in enumerate(delays):
                assert got[s] == want[dl], (scheme, s)
                st = rx.state(s)
                assert st["dropped"] == 0 and st["cut_hits"] == 0 and st["base"] + st["fill"] == \
                    (len(recs[s]) - N) // HOP + 1


def test_stereo_downmix_and_lead_in(A, torch, handle):
    K, fec, lead = 2, 0, 312
    d = handle(K)
    pcm, word, Nsym, rxcfg, datas = rx_setup(A, K, fec, n_frames=3)
    want = one_shot(d, pcm, word, Nsym, fec)
    rng = np.random.default_rng(8)
    e = rng.integers(-900, 901, len(pcm)).astype(np.int32)
    stereo = np.stack([pcm + e, pcm - e], axis=1)                  # (L + R) >> 1 is pcm
    assert np.abs(stereo).max() < 32768
    junk = rng.integers(-20000, 20001, (lead, 2))
    rec = np.concatenate([junk, stereo]).astype(np.int16).reshape(-1)
    with A.Receiver(1, rxcfg, n=N, hop=HOP, freqs=tones(K), channels=2, channel_mode=A.CH_DOWNMIX,
                    lead_in=lead) as rx:
        got = run_streams(rx, [rec], [packets_of(len(rec) // 2, "ragged", 5)], ch=2)
    assert got[0] == want and [b for _, _, b in want] == datas


def detector_pieces(d, pcm, sizes):
    """The detector's outputs of the recording, cut as a receiver that is pushed
    packets of `sizes` frames sees them: [(sym, P)] per push."""
    W = (len(pcm) - N) // HOP + 1
    sym, P = d.batch(pcm[:(W - 1) * HOP + N], mags=True)
    return LR.pieces(sym, P, sizes, N, HOP)


@pytest.mark.parametrize("fec", [0, 1])
def test_ring_overflow(A, torch, handle, fec):
    """ring_windows at its minimum and a first packet that overflows it: dropped
    and every later frame as the reference receiver gives them on the detector's
    own outputs."""
    K = 2
    d = handle(K)
    pcm, word, Nsym, rxcfg, datas = rx_setup(A, K, fec, n_frames=4)
    ring = X.min_ring(L_WORD, Nsym, R)
    rxcfg.ring_windows = ring
    big = (ring + 3 * (L_WORD + Nsym)) * HOP
    sizes = [big] + packets_of(len(pcm) - big, "packets")
    ref = X.Rx(1, K, R, word, 0, Nsym, H, KIND, fec, 8, ring)
    want, dropped = [], []
    for piece in detector_pieces(d, pcm, sizes):
        fr, bodies, _ = ref.push([piece])
        want += [(int(f["window"]), int(f["errors"]), b) for f, b in zip(fr, bodies)]
        dropped.append(int(ref.state["dropped"][0]))
    assert dropped[0] > 0 and dropped[-1] == dropped[0]
    with A.Receiver(1, rxcfg, n=N, hop=HOP, freqs=tones(K)) as rx:
        got = run_streams(rx, [pcm], [sizes])
        st = rx.state(0)
    assert got[0] == want and 1 <= len(want) < len(datas), "a frame is lost to the overflow, a later one received"
    assert st["dropped"] == dropped[-1] and st["cut_hits"] == 0
    assert {k: int(ref.state[k][0]) for k in st} == st


def test_max_frames_cuts(A, torch, handle):
    """max_frames = 1 and two frames completing in one push: the first comes
    back, cut_hits says that one did not."""
    K, fec = 2, 0
    d = handle(K)
    pcm, word, Nsym, rxcfg, datas = rx_setup(A, K, fec, max_frames=1, n_frames=2)
    want = one_shot(d, pcm, word, Nsym, fec)
    assert len(want) == 2
    with A.Receiver(1, rxcfg, n=N, hop=HOP, freqs=tones(K)) as rx:
        got = run_streams(rx, [pcm], [[len(pcm)]])
        assert got[0] == want[:1] and rx.state(0)["cut_hits"] == 1


def test_reset_one_of_three(A, torch, handle):
    """demod_rx_reset of stream 1 in the middle of its second frame: that frame
    is missing, its later frames count from the reset, the others are intact."""
    K, fec = 2, 0
    d = handle(K)
    pcm, word, Nsym, rxcfg, datas = rx_setup(A, K, fec, n_frames=4)
    want = one_shot(d, pcm, word, Nsym, fec)
    assert len(want) == 4
    cut = (want[1][0] + (L_WORD + 8) * R) * HOP                    # samples: inside frame 1's payload
    head, tail = [pcm[:cut]] * 3, [pcm[cut:]] * 3
    with A.Receiver(3, rxcfg, n=N, hop=HOP, freqs=tones(K)) as rx:
        a = run_streams(rx, head, [packets_of(cut, "packets")] * 3)
        assert rx.state(1)["fill"] > 0
        rx.reset(1)
        assert rx.state(1) == dict(base=0, hold=0, dropped=0, cut_hits=0, fill=0, keep=0)
        assert rx.state(0)["fill"] > 0
        b = run_streams(rx, tail, [packets_of(len(pcm) - cut, "packets")] * 3)
        with pytest.raises(A.DemodError):
            rx.reset(3)
        with pytest.raises(A.DemodError):
            rx.state(3)
    for s in (0, 2):
        assert a[s] + b[s] == want
    assert a[1] == want[:1] and b[1] == one_shot(d, pcm[cut:], word, Nsym, fec)
    assert [x[2] for x in b[1]] == datas[2:]


def test_push_refusals_consume_nothing(A, torch, handle):
    K, fec = 2, 0
    d = handle(K)
    pcm, word, Nsym, rxcfg, datas = rx_setup(A, K, fec, n_frames=2)
    want = one_shot(d, pcm, word, Nsym, fec)
    lib = A.load_library()
    half = len(pcm) // 2
    with A.Receiver(2, rxcfg, n=N, hop=HOP, freqs=tones(K)) as rx:
        a = run_streams(rx, [pcm[:half]] * 2, [[half]] * 2)
        before = [rx.state(s) for s in range(2)]
        fr, bo, su = ctypes.c_void_p(), ctypes.c_void_p(), A.DemodRxSummary()
        ptrs = np.array([pcm.ctypes.data, 0], np.uintp)
        nfr = np.array([100, 100], np.uintp)
        args = (ptrs.ctypes.data, nfr.ctypes.data, ctypes.byref(fr), ctypes.byref(bo), ctypes.byref(su))
        assert lib.demod_rx_push(rx._h, *args) == A.DEMOD_BAD_ARG                 # a missing packet
        nfr[1] = 0
        nfr[0] = 2 ** 41
        assert lib.demod_rx_push(rx._h, *args) == A.DEMOD_BAD_ARG                 # an absurd length
        nfr[0] = 100
        for i in (0, 1, 2, 3, 4):
            bad = list(args)
            bad[i] = None
            assert lib.demod_rx_push(rx._h, *bad) == A.DEMOD_BAD_ARG, i
        assert lib.demod_rx_push(None, *args) == A.DEMOD_BAD_ARG
        with pytest.raises(A.DemodError):
            rx.push([pcm[:10]])                                                   # one packet per stream
        assert [rx.state(s) for s in range(2)] == before
        b = run_streams(rx, [pcm[half:]] * 2, [[len(pcm) - half]] * 2)
    assert a[0] + b[0] == want and a[1] + b[1] == want
    # what demod_rx_create refuses comes back as demod_rx_sizes' code
    for kw in (dict(ring_windows=X.min_ring(L_WORD, Nsym, R) - 1), dict(max_frames=0), dict(crc=0)):
        bad = A.make_rx_cfg(word, 0, Nsym, H, KIND, fec, 8, 10 ** 4)
        for k, v in kw.items():
            setattr(bad, k, v)
        with pytest.raises(A.DemodError) as e:
            A.Receiver(2, bad, n=N, hop=HOP, freqs=tones(K))
        assert e.value.code == A.DEMOD_BAD_ARG
    with pytest.raises(A.DemodError):
        A.Receiver(0, rxcfg, n=N, hop=HOP, freqs=tones(K))
