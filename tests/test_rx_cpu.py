"""The receiver without a GPU (include/demod.h "receiver"): the ABI (exports,
struct layouts, NULL arguments), demod_rx_sizes against tests/rx_ref.py's closed
forms with every refusal, what the Python mirror refuses before a pointer
reaches the library, and the property the definitions exist for: the frames the
reference receiver emits over all pushes, whatever the piece sizes, are the kept
frames of the one-shot check (or decode and check) on the whole recording."""
import ctypes

import numpy as np
import pytest

import frames_check_ref as C
import frames_ref as F
import rx_ref as X

EXPORTS = ("demod_rx_sizes", "demod_rx_advance_async", "demod_rx_collect_workspace_size",
           "demod_rx_collect_async", "demod_rx_create", "demod_rx_destroy", "demod_rx_reset", "demod_rx_state",
           "demod_rx_push")
FSK8 = F.FSK8


def test_exports_and_mirror(A):
    lib = A.load_library()
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in A.header_exports()
        assert getattr(lib, name).argtypes is not None, name
    for name in ("rx_advance_async", "rx_collect_async"):
        assert callable(getattr(A.Demodulator, name))
    for name in ("push", "reset", "state", "close"):
        assert callable(getattr(A.Receiver, name))
    assert callable(A.rx_sizes) and callable(A.rx_collect_workspace_size) and callable(A.make_rx_cfg)


def test_struct_layouts(A):
    Fr, St, Su, Cf, Sz = A.DemodRxFrame, A.DemodRxStreamState, A.DemodRxSummary, A.DemodRxCfg, A.DemodRxSizes
    assert (ctypes.sizeof(Fr), ctypes.sizeof(St), ctypes.sizeof(Su)) == (32, 40, 32)
    assert [getattr(Fr, f).offset for f, _ in Fr._fields_] == [0, 4, 8, 16, 24, 28]
    assert [getattr(St, f).offset for f, _ in St._fields_] == [0, 8, 16, 24, 32, 36]
    assert [getattr(Su, f).offset for f, _ in Su._fields_] == [0, 8, 16, 24]
    assert ctypes.sizeof(Cf) == 64 + 8 * 4 and Cf.sync_len.offset == 64 and Cf.ring_windows.offset == 92
    assert ctypes.sizeof(Sz) == 72
    assert A.RX_FRAME_DTYPE == X.FRAME_DTYPE and A.RX_STATE_DTYPE == X.STATE_DTYPE
    assert A.RX_SUMMARY_DTYPE == X.SUMMARY_DTYPE
    for dt, T in ((A.RX_FRAME_DTYPE, Fr), (A.RX_STATE_DTYPE, St), (A.RX_SUMMARY_DTYPE, Su)):
        assert dt.itemsize == ctypes.sizeof(T)
        assert [dt.fields[f][1] for f, _ in T._fields_] == [getattr(T, f).offset for f, _ in T._fields_]
    assert X.RESULT_DTYPE.itemsize == ctypes.sizeof(A.DemodFramesResult)


def test_null_arguments(A):
    lib = A.load_library()
    assert lib.demod_rx_advance_async(None, None, None, None, None, None, 0, None, None, 1, 96, None, None, None,
                                      None, None) == A.DEMOD_BAD_ARG
    assert lib.demod_rx_collect_async(None, None, None, None, None, None, None, None, 1, 1, 8, 64, 1, 1, 0, None,
                                      None, None, None, 0, None) == A.DEMOD_BAD_ARG
    assert lib.demod_rx_push(None, None, None, None, None, None) == A.DEMOD_BAD_ARG
    assert lib.demod_rx_reset(None, 0) == A.DEMOD_BAD_ARG
    assert lib.demod_rx_state(None, 0, None) == A.DEMOD_BAD_ARG
    lib.demod_rx_destroy(None)
    err = ctypes.c_int(0)
    assert not lib.demod_rx_create(None, None, 1, ctypes.byref(err)) and err.value == A.DEMOD_BAD_ARG
    cfg = A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS)
    out = A.DemodRxSizes()
    assert lib.demod_rx_sizes(ctypes.byref(cfg), None, 1, ctypes.byref(out)) == A.DEMOD_BAD_ARG
    assert lib.demod_rx_sizes(None, ctypes.byref(A.DemodRxCfg()), 1, ctypes.byref(out)) == A.DEMOD_BAD_ARG
    assert lib.demod_rx_collect_workspace_size(None, 4) == 0


SIZE_CASES = [  # freqs, hop, S, L, N, h, kind, fec, max_frames, ring (None: the minimum)
    (F.FSK2, 256, 1, 24, 64, 1, C.CRC16, 0, 1, None),
    (F.FSK2, 256, 1024, 16, 128, 2, C.CRC32, 0, 4, 1200),
    (FSK8, 256, 65, 8, 90, 2, C.CRC16, 0, 16, None),
    (FSK8, 1024, 3, 8, 40, 1, C.CRC16, 0, 2, 200),
    (F.FSK2, 256, 1024, 24, 400, 2, C.CRC16, 1, 4, None),
    (FSK8, 256, 20000, 12, 60, 1, C.CRC32, 1, 3, None),
    (FSK8, 512, 65536, 12, 64, 1, C.CRC16, 1, 1, 400),
]


@pytest.mark.parametrize("case", SIZE_CASES)
def test_sizes_closed_forms(A, case):
    freqs, hop, S, L, N, h, kind, fec, mf, ring = case
    cfg = A.make_cfg(n=1024, hop=hop, freqs=freqs)
    K, R = len(freqs), 1024 // hop
    ring = ring or X.min_ring(L, N, R)
    rx = A.make_rx_cfg(np.arange(L) % K, 1, N, h, kind, fec, mf, ring)
    got = A.rx_sizes(cfg, rx, S)
    assert got == X.sizes(K, R, S, L, N, h, kind, fec, mf, ring)
    assert got["scan_work_bytes"] == A.frames_segments_workspace_size(cfg, S, S * ring)
    assert got["collect_work_bytes"] == A.rx_collect_workspace_size(cfg, S) == X.collect_work_bytes(S)
    if fec:
        assert got["decode_work_bytes"] == A.frames_decode_workspace_size(cfg, S, mf, N)


def test_sizes_refusals(A):
    cfg = A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS)
    K, R, L, N = 2, 4, 16, 64
    base = dict(sync=np.arange(L) % K, max_errors=1, frame_symbols=N, len_bytes=1, crc=C.CRC16, fec=0,
                max_frames=4, ring_windows=X.min_ring(L, N, R))

    def refused(S=8, cfg=cfg, **kw):
        a = dict(base)
        a.update(kw)
        with pytest.raises(A.DemodError) as e:
            A.rx_sizes(cfg, A.make_rx_cfg(**a), S)
        assert e.value.code == A.DEMOD_BAD_ARG
        return True

    assert A.rx_sizes(cfg, A.make_rx_cfg(**base), 8)["max_len"] == 5
    # the streams and the rows
    assert refused(S=0) and refused(S=A.DEMOD_MAX_SEGMENTS + 1) and refused(max_frames=0)
    assert refused(S=2 ** 15, max_frames=2 ** 16)
    # the ring: below 2 (L + N) R, S C at or above 2^31
    assert refused(ring_windows=X.min_ring(L, N, R) - 1) and refused(ring_windows=0)
    assert refused(S=2 ** 16, ring_windows=2 ** 15) and refused(S=3, ring_windows=2 ** 31 // 3 + 1)
    assert refused(S=1, ring_windows=2 ** 31)
    A.rx_sizes(cfg, A.make_rx_cfg(**dict(base, ring_windows=2 ** 15 - 1)), 2 ** 16)
    # what the scan refuses: the word, (L + N) R
    assert refused(sync=[]) and refused(max_errors=L) and refused(sync=[0, 1, 2, 1])
    assert refused(frame_symbols=2 ** 29, ring_windows=2 ** 31 - 1, S=1)
    # what the check refuses: the header, the CRC kind, the row shape
    assert refused(len_bytes=0) and refused(len_bytes=3) and refused(crc=0) and refused(crc=3)
    assert refused(frame_symbols=16) and refused(frame_symbols=8 * 4200, ring_windows=2 ** 20)
    # what the decode refuses: the code, K not a power of two, rows below the look-ahead
    assert refused(fec=2) and refused(fec=1, frame_symbols=64)
    k3 = A.make_cfg(n=1024, hop=256, freqs=(1500.0, 2250.0, 3000.0))
    assert refused(cfg=k3, fec=1, frame_symbols=200, ring_windows=4000)
    A.rx_sizes(k3, A.make_rx_cfg(**dict(base, frame_symbols=200, ring_windows=4000)), 8)
    # the configuration
    bad = A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS)
    bad.hop = 12
    assert refused(cfg=bad)
    with pytest.raises(A.DemodError):
        A.make_rx_cfg(np.zeros(A.DEMOD_MAX_SYNC + 1, np.uint8))
    with pytest.raises(A.DemodError):
        A.rx_collect_workspace_size(cfg, 0)
    with pytest.raises(A.DemodError):
        A.rx_collect_workspace_size(cfg, A.DEMOD_MAX_SEGMENTS + 1)


def test_python_mirror_refuses_before_the_library(A):
    """No device here: every path of the two async mirrors ends in their own checks."""
    torch = pytest.importorskip("torch")
    d = object.__new__(A.Demodulator)
    d._lib, d.cfg, d._h = A.load_library(), A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS), None
    S, Cw, mf, N = 2, 96, 4, 64

    def t(n, dtype=torch.uint8):
        return torch.zeros(n, dtype=dtype)

    def adv(**kw):
        a = dict(d_state=t(S * 40), d_ring_sym_in=t(S * Cw), d_ring_mag_in=t(S * Cw * 2, torch.float32),
                 d_new_sym=t(10), d_new_mag=t(20, torch.float32), n_new_windows=10,
                 d_new_first=t(S, torch.int64), d_new_count=t(S, torch.int32), n_streams=S, ring_windows=Cw,
                 d_ring_sym_out=t(S * Cw), d_ring_mag_out=t(S * Cw * 2, torch.float32),
                 d_first=t(S, torch.int64), d_count=t(S, torch.int32))
        a.update(kw)
        with pytest.raises(A.DemodError) as e:
            d.rx_advance_async(**a)
        assert e.value.code == A.DEMOD_BAD_ARG
        return str(e.value)

    def col(**kw):
        a = dict(d_state=t(S * 40), d_hits=t(S * mf * 16), d_results=t(S * 560), d_check=t(S * mf * 16),
                 d_kept=t(S * mf, torch.int32), d_body=t(S * mf * 5), d_check_summary=t(S * 32), n_streams=S,
                 max_frames=mf, sync_len=8, frame_symbols=N, len_bytes=1, crc=C.CRC16, fec=0,
                 d_frames=t(S * mf * 32), d_bodies=t(S * mf * 5), d_summary=t(32), d_work=t(48))
        a.update(kw)
        with pytest.raises(A.DemodError) as e:
            d.rx_collect_async(**a)
        assert e.value.code == A.DEMOD_BAD_ARG
        return str(e.value)

    assert "d_state" in adv() and "d_state" in col()       # host tensors: the first one is refused
    for kw in (dict(n_streams=0), dict(n_streams=A.DEMOD_MAX_SEGMENTS + 1), dict(ring_windows=0),
               dict(n_streams=2 ** 16, ring_windows=2 ** 15), dict(n_new_windows=-1), dict(n_new_windows=2 ** 31)):
        assert "n_streams" in adv(**kw)
    for kw in (dict(n_streams=0), dict(max_frames=0), dict(n_streams=2 ** 15, max_frames=2 ** 16),
               dict(frame_symbols=-1)):
        assert "n_streams" in col(**kw)
    assert "fec" in col(fec=2) and "len_bytes" in col(crc=9) and "rows too short" in col(frame_symbols=16)
    assert "look-ahead" in col(fec=1)
    assert "raw address" in adv(d_state=1234) and "required" in col(d_state=None)


# ---- the reference against the one-shot check ---------------------------------------

L_WORD, H, KIND, P0 = 16, 1, C.CRC16, 2
DATA = (b"abc", b"", b"hello")


def pieces_of(W, scheme, seed=0):
    """Piece lengths that add up to W."""
    if scheme == "one":
        return [W]
    if scheme == "eleven":
        return [11] * (W // 11) + ([W % 11] if W % 11 else [])
    rng = np.random.default_rng(seed)
    out, left = [0, 1], W - 1
    while left:
        p = int(min(left, rng.choice([0, 1, 2, 5, 17, 40, 90])))
        out.append(p)
        left -= p
    return out


def run_pieces(sym, P, K, R, word, N, fec, cuts, ring, max_frames=16):
    rx = X.Rx(1, K, R, word, 0, N, H, KIND, fec, max_frames, ring)
    out, at = [], 0
    for n in cuts:
        fr, bodies, summ = rx.push([(sym[at:at + n], P[at:at + n])])
        assert summ["n_frames"] == len(fr) == len(bodies) and summ["n_bytes"] == sum(map(len, bodies))
        assert [int(b) for b in fr["body"]] == np.cumsum([0] + [len(b) for b in bodies])[:-1].tolist()
        out += [(int(f["window"]), int(f["errors"]), b) for f, b in zip(fr, bodies)]
        at += n
    assert at == len(sym)
    st = rx.state[0]
    assert st["dropped"] == 0 and st["cut_hits"] == 0
    assert set(rx.phases[0]) <= {P0 % R}, "the fixture holds the absolute phase at every push"
    return out


def recording(K, R, fec, items, seed):
    rng = np.random.default_rng(seed)
    bits = F.bits_per_symbol(K)
    word = rng.integers(0, K, L_WORD).astype(np.uint8)
    N = X.row_symbols(H, KIND, fec, bits, 5)
    symbols, planted = X.stream_symbols(list(items) + [N + 3], K, word, H, KIND, fec, rng)
    sym, P = X.windows_of(symbols, K, R, P0, rng)
    return sym, P, word, N, [(P0 + a * R, d) for a, d in planted]


@pytest.mark.parametrize("fec", [0, 1])
@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("K", [2, 8])
def test_pieces_give_the_one_shot_frames(K, R, fec):
    """Three frames; the recording in one piece, in pieces of 11 windows (with
    the smallest ring too) and in seeded ragged pieces that include 0 and 1."""
    sym, P, word, N, planted = recording(K, R, fec, [7, DATA[0], 5, DATA[1], 9, DATA[2]], 100 * K + 10 * R + fec)
    whole = X.one_shot(sym, P, R, word, 0, N, H, KIND, fec)
    assert [(w, 0, d) for w, d in planted] == whole
    W = len(sym)
    for scheme in ("one", "eleven", "ragged"):
        assert run_pieces(sym, P, K, R, word, N, fec, pieces_of(W, scheme, 7), W + 5) == whole, scheme
    assert run_pieces(sym, P, K, R, word, N, fec, pieces_of(W, "eleven"), X.min_ring(L_WORD, N, R)) == whole


@pytest.mark.parametrize("fec", [0, 1])
@pytest.mark.parametrize("K", [2, 8])
def test_boundaries_and_touching_frames(K, fec):
    """A frame (its row, and its own span) ending exactly on a piece boundary
    and one window to either side; the word split across two pieces at every
    symbol; two touching frames."""
    R = 4
    bits = F.bits_per_symbol(K)
    sym, P, word, N, planted = recording(K, R, fec, [6, DATA[2], DATA[0], 4, DATA[1]], 900 + K + fec)
    whole = X.one_shot(sym, P, R, word, 0, N, H, KIND, fec)
    assert [(w, 0, d) for w, d in planted] == whole
    (w0, d0), (w1, _), _ = planted
    assert w1 == w0 + (L_WORD + X.span(len(d0), bits, H, KIND, fec)) * R      # touching
    W = len(sym)
    row_end = w0 + (L_WORD + N - 1) * R + 1          # the first length at which frame 0 is complete
    cuts = [row_end - 1, row_end, row_end + 1, w1 - 1, w1, w1 + 1]
    cuts += [w1 + j * R + d for j in range(L_WORD) for d in (0, 1)]       # inside the second frame's word
    for cut in cuts:
        assert run_pieces(sym, P, K, R, word, N, fec, [cut, W - cut], W) == whole, cut
        assert run_pieces(sym, P, K, R, word, N, fec, [cut, 1, 0, W - cut - 1], W) == whole, cut


@pytest.mark.parametrize("K", [2, 8])
def test_hold_rule(K):
    """A valid short frame inside a longer valid frame's span. The one-shot
    check drops it as covered; in pieces the long frame is emitted pushes before
    the short one completes, and `hold` is what still drops it. (Plain frames: a
    coded frame's bits cannot carry another frame's symbols.)"""
    R, fec = 4, 0
    bits = F.bits_per_symbol(K)
    rng = np.random.default_rng(31 + K)
    word = rng.integers(0, K, L_WORD).astype(np.uint8)
    inner = X.frame_symbols(b"in", word, bits, H, KIND, fec)
    outer = X.embed(inner, bits, H)
    N = X.row_symbols(H, KIND, fec, bits, len(outer))
    symbols, planted = X.stream_symbols([5, outer, 3, b"next", N + 3], K, word, H, KIND, fec, rng)
    sym, P = X.windows_of(symbols, K, R, P0, rng)
    w_out = P0 + planted[0][0] * R
    w_in = w_out + (L_WORD + 8) * R
    hits, check, kept, _, _, _ = X.scan_check(sym, P, R, word, 0, N, H, KIND, fec)
    rows = {int(w): i for i, w in enumerate(hits["window"])}
    assert check["status"][rows[w_in]] == C.OK and check["covered"][rows[w_in]] == 1
    whole = X.one_shot(sym, P, R, word, 0, N, H, KIND, fec)
    assert [(w, d) for w, _, d in whole] == [(w_out, outer), (P0 + planted[1][0] * R, b"next")]
    W = len(sym)
    for scheme in ("one", "eleven", "ragged"):
        assert run_pieces(sym, P, K, R, word, N, fec, pieces_of(W, scheme, 3), W + 5) == whole, scheme
    # the push that completes the outer frame and not yet the inner one
    cut = w_out + (L_WORD + N - 1) * R + 1
    rx = X.Rx(1, K, R, word, 0, N, H, KIND, fec, 16, W)
    fr, _, _ = rx.push([(sym[:cut], P[:cut])])
    assert fr["window"].tolist() == [w_out] and rx.state["keep"][0] == w_in - (R - 1) - rx.state["base"][0]
    assert rx.state["hold"][0] == w_out + (L_WORD + X.span(len(outer), bits, H, KIND, fec)) * R > w_in
    fr, _, summ = rx.push([(sym[cut:], P[cut:])])
    assert fr["window"].tolist() == [P0 + planted[1][0] * R] and summ["n_valid"] == 2


def test_ring_overflow_and_cut(A):
    """The counters the equality above excludes: a piece larger than the ring
    drops the oldest windows, max_frames = 1 cuts the second frame of a push."""
    K, R, fec = 2, 4, 0
    sym, P, word, N, planted = recording(K, R, fec, [7, DATA[0], 5, DATA[1], 9, DATA[2]], 5)
    W, ring = len(sym), X.min_ring(L_WORD, N, R)
    rx = X.Rx(1, K, R, word, 0, N, H, KIND, fec, 16, ring)
    fr, bodies, _ = rx.push([(sym, P)])
    st = rx.state[0]
    assert st["dropped"] == W - ring and st["base"] == W - ring and st["fill"] == ring
    assert [(int(f["window"]), b) for f, b in zip(fr, bodies)] == [p for p in planted if p[0] >= W - ring
                                                                  and p[0] + (L_WORD + N) * R <= W]
    rx = X.Rx(1, K, R, word, 0, N, H, KIND, fec, 1, W)
    fr, bodies, _ = rx.push([(sym, P)])
    assert rx.state["cut_hits"][0] == 2 and [(int(f["window"]), b) for f, b in zip(fr, bodies)] == planted[:1]
