"""The transmitter without a device (include/demod.h "transmitter"): the frame's
symbols (csrc/demod_tx_frame.c) against tests/tx_ref.py, demod_tx_sizes'
refusals and closed forms, the reference modulator cut into pieces, the
reference signal through the oracle detector and the frame references (the
inputs of the GPU loopback test, fixed here as ones whose frames all come back),
and the host sources in a standalone program under AddressSanitizer and UBSan
(tests/native/tx_host_test.c)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import frames_check_ref as C
import rx_ref as X
import tx_ref as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXPORTS = ("demod_tx_frame_symbol_count", "demod_tx_frame_symbols", "demod_tx_sizes", "demod_tx_encode_async",
           "demod_tx_modulate_workspace_size", "demod_tx_modulate_async", "demod_tx_create", "demod_tx_destroy",
           "demod_tx_reset", "demod_tx_state", "demod_tx_device_buffers", "demod_tx_send", "demod_tx_pull")


@pytest.fixture(scope="module")
def lut(O):
    return O.sine_lut()


def tones(K):
    return T.loop_tones(K)


def test_exports_and_mirror(A):
    lib = A.load_library()
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in A.header_exports()
        assert getattr(lib, name).argtypes is not None, name
    for name in ("tx_encode_async", "tx_modulate_async"):
        assert callable(getattr(A.Demodulator, name))
    for name in ("send", "pull", "reset", "state", "close", "device_buffers"):
        assert callable(getattr(A.Transmitter, name))
    assert callable(A.tx_sizes) and callable(A.tx_frame_symbols) and callable(A.make_tx_cfg)


def test_struct_layouts(A):
    Cf, St, Pl, Sz = A.DemodTxCfg, A.DemodTxStreamState, A.DemodTxPlace, A.DemodTxSizes
    assert (ctypes.sizeof(Cf), ctypes.sizeof(St), ctypes.sizeof(Pl), ctypes.sizeof(Sz)) == (184, 40, 16, 64)
    assert [getattr(Cf, f).offset for f, _ in Cf._fields_] == [0, 64, 68, 72, 76, 80, 84, 88, 152, 156, 160, 164,
                                                                168, 176, 180]
    assert A.TX_STATE_DTYPE == T.STATE_DTYPE and A.TX_PLACE_DTYPE == T.PLACE_DTYPE
    assert A.TX_RECORD_DTYPE == T.RECORD_DTYPE
    for dt, Ty in ((A.TX_STATE_DTYPE, St), (A.TX_PLACE_DTYPE, Pl)):
        assert dt.itemsize == ctypes.sizeof(Ty)
        assert [dt.fields[f][1] for f, _ in Ty._fields_] == [getattr(Ty, f).offset for f, _ in Ty._fields_]
    assert (A.DEMOD_TX_OK, A.DEMOD_TX_BAD_LENGTH, A.DEMOD_TX_NO_ROOM) == (T.OK, T.BAD_LENGTH, T.NO_ROOM)


def test_null_arguments(A):
    lib = A.load_library()
    x = A.DemodTxCfg()
    assert lib.demod_tx_encode_async(None, ctypes.byref(x), None, None, None, None, None, 0, 1, None,
                                     None) == A.DEMOD_BAD_ARG
    assert lib.demod_tx_modulate_async(None, ctypes.byref(x), None, None, None, 1, None, None, 0,
                                       None) == A.DEMOD_BAD_ARG
    assert lib.demod_tx_send(None, None, 0, None, 0, None) == A.DEMOD_BAD_ARG
    assert lib.demod_tx_pull(None, None, None) == A.DEMOD_BAD_ARG
    assert lib.demod_tx_reset(None, 0) == A.DEMOD_BAD_ARG
    assert lib.demod_tx_state(None, 0, None) == A.DEMOD_BAD_ARG
    assert lib.demod_tx_device_buffers(None, None, None) == A.DEMOD_BAD_ARG
    lib.demod_tx_destroy(None)
    err = ctypes.c_int(0)
    assert not lib.demod_tx_create(None, None, 1, ctypes.byref(err)) and err.value == A.DEMOD_BAD_ARG
    cfg = A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS)
    out = A.DemodTxSizes()
    assert lib.demod_tx_sizes(ctypes.byref(cfg), None, 1, ctypes.byref(out)) == A.DEMOD_BAD_ARG
    assert lib.demod_tx_sizes(None, ctypes.byref(x), 1, ctypes.byref(out)) == A.DEMOD_BAD_ARG
    assert lib.demod_tx_modulate_workspace_size(None, ctypes.byref(x), 4) == 0


# ---- the frame's symbols -------------------------------------------------------------

@pytest.mark.parametrize("fec", [0, 1])
@pytest.mark.parametrize("kind", [C.CRC16, C.CRC32])
@pytest.mark.parametrize("h", [1, 2])
@pytest.mark.parametrize("K", [2, 4, 8, 16])
def test_frame_symbols(A, lut, K, h, kind, fec):
    """Lengths 0, 1, both sides of 8 (h + len + c) + 6 = 8 h + 64 (where the
    coded frame leaves its zero fill: len + c = 7 and 8), max_len; max_len + 1
    is refused."""
    rng = np.random.default_rng(100 * K + 10 * h + kind + fec)
    max_len = 255 if h == 1 else 300
    word = rng.integers(0, K, 24).astype(np.uint8)
    c = T.make(tones(K), 1024, lut, word, h=h, kind=kind, fec=fec, max_len=max_len)
    x = A.make_tx_cfg(word, len_bytes=h, crc=kind, fec=fec, max_len=max_len)
    cb = C.CRC_BYTES[kind]
    for ln in (0, 1, 7 - cb, 8 - cb, max_len):
        data = rng.integers(0, 256, ln).astype(np.uint8).tobytes()
        want = T.frame_symbols(c, data)
        assert A.tx_frame_symbol_count(x, K, ln) == len(want) == T.frame_count(c, ln)
        got = A.tx_frame_symbols(x, K, data)
        assert np.array_equal(got, want), (ln, np.flatnonzero(got != want)[:8])
        assert np.array_equal(got[:24], word) and int(got.max()) < K
    with pytest.raises(A.DemodError) as e:
        A.tx_frame_symbols(x, K, bytes(max_len + 1))
    assert e.value.code == A.DEMOD_FRAME_TOO_LARGE


def test_frame_symbols_refusals(A):
    base = dict(sync=[0, 1, 1, 0], len_bytes=1, crc=C.CRC16, fec=0, max_len=8)

    def refused(k=4, data=b"ab", **kw):
        with pytest.raises(A.DemodError) as e:
            A.tx_frame_symbols(A.make_tx_cfg(**dict(base, **kw)), k, data)
        assert e.value.code == A.DEMOD_BAD_ARG, kw
        return True

    assert len(A.tx_frame_symbols(A.make_tx_cfg(**base), 4, b"ab")) == 4 + 20
    assert refused(k=1) and refused(k=17) and refused(sync=[]) and refused(sync=[0, 4])
    assert refused(len_bytes=0) and refused(len_bytes=3) and refused(crc=0) and refused(crc=3)
    assert refused(fec=2) and refused(k=3, fec=1) and refused(k=12, fec=1)
    assert len(A.tx_frame_symbols(A.make_tx_cfg(**base), 3, b"ab")) == 4 + 20   # K = 3 without the code: 2 bits
    with pytest.raises(A.DemodError) as e:   # max_len above what one length byte can say
        A.tx_frame_symbols(A.make_tx_cfg(**dict(base, max_len=400)), 4, bytes(256))
    assert e.value.code == A.DEMOD_FRAME_TOO_LARGE


# ---- demod_tx_sizes --------------------------------------------------------------------

SIZE_CASES = [  # K, n, S, L, h, kind, fec, max_len, gap, ring (None: the minimum), max_frames, stride
    (2, 1024, 1, 16, 1, C.CRC16, 0, 3, 0, None, 1, 8),
    (2, 1024, 1024, 24, 2, C.CRC32, 0, 64, 3, 2000, 4, 2880),
    (8, 256, 65, 8, 2, C.CRC16, 1, 40, 1, None, 130, 2888),
    (16, 64, 65536, 1, 1, C.CRC16, 1, 0, 0, 400, 1, 64),
    (4, 4096, 3, 64, 2, C.CRC32, 1, 4096, 7, None, 5, 2 ** 20),
    (3, 1024, 7, 5, 2, C.CRC16, 0, 4096, 0, None, 2, 1016),
]


@pytest.mark.parametrize("case", SIZE_CASES)
def test_sizes_closed_forms(A, lut, case):
    K, n, S, L, h, kind, fec, max_len, gap, ring, mf, stride = case
    freqs = tuple(1000.0 + 300.0 * i for i in range(K))
    cfg = A.make_cfg(n=n, hop=n // 4, freqs=freqs)
    word = np.arange(L) % K
    c = T.make(freqs, n, lut, word, h=h, kind=kind, fec=fec, max_len=max_len, gap=gap, ring=ring, max_frames=mf,
               stride=stride)
    x = A.make_tx_cfg(word, h, kind, fec, max_len, gap, ring_symbols=c.C, max_frames=mf, max_samples=stride)
    got = A.tx_sizes(cfg, x, S)
    assert got == T.sizes(c, S)
    assert got["max_symbols"] == A.tx_frame_symbol_count(x, K, max_len)
    assert got["modulate_work_bytes"] == A.tx_modulate_workspace_size(cfg, x, S) \
        == 4 * S * ((n - 1 + stride) // n + 2)


def test_sizes_refusals(A):
    cfg = A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS)
    base = dict(sync=[0, 1, 1, 0], len_bytes=1, crc=C.CRC16, fec=0, max_len=5, gap=2, idle=[0, 1], amplitude=8000,
                sigma=400, seed=1, ring_symbols=4 + 64 + 2, max_frames=4, max_samples=2880)

    def refused(S=8, cfg=cfg, **kw):
        with pytest.raises(A.DemodError) as e:
            A.tx_sizes(cfg, A.make_tx_cfg(**dict(base, **kw)), S)
        assert e.value.code == A.DEMOD_BAD_ARG, kw
        return True

    assert A.tx_sizes(cfg, A.make_tx_cfg(**base), 8)["max_symbols"] == 4 + 8 * (1 + 5 + 2)
    # the word and the idle pattern
    assert refused(sync=[]) and refused(sync=[0, 2]) and refused(idle=[]) and refused(idle=[1, 0, 2])
    # the format
    assert refused(len_bytes=0) and refused(len_bytes=3) and refused(crc=0) and refused(crc=3) and refused(fec=2)
    k3 = A.make_cfg(n=1024, hop=256, freqs=(1500.0, 2250.0, 3000.0))
    assert refused(cfg=k3, fec=1, ring_symbols=4000)
    A.tx_sizes(k3, A.make_tx_cfg(**dict(base, ring_symbols=4000)), 8)
    # max_len: above 256^h - 1, above DEMOD_MAX_FRAME_PAYLOAD
    assert refused(max_len=256, ring_symbols=10 ** 4)
    assert refused(len_bytes=2, max_len=A.DEMOD_MAX_FRAME_PAYLOAD + 1, ring_symbols=10 ** 5)
    A.tx_sizes(cfg, A.make_tx_cfg(**dict(base, len_bytes=2, max_len=A.DEMOD_MAX_FRAME_PAYLOAD,
                                         ring_symbols=10 ** 5)), 8)
    # the ring: below A(max_len) + gap, S C at or above 2^31
    assert refused(ring_symbols=4 + 64 + 1) and refused(ring_symbols=0)
    assert refused(S=2 ** 16, ring_symbols=2 ** 15) and refused(S=1, ring_symbols=2 ** 31)
    A.tx_sizes(cfg, A.make_tx_cfg(**dict(base, ring_symbols=2 ** 15 - 1, max_samples=8)), 2 ** 16)
    # the streams and the frames
    assert refused(S=0) and refused(S=A.DEMOD_MAX_SEGMENTS + 1) and refused(max_frames=0)
    assert refused(S=2 ** 15, max_frames=2 ** 16, max_samples=8)
    # the stride
    assert refused(max_samples=0) and refused(max_samples=2884) and refused(S=2 ** 16, max_samples=2 ** 15)
    assert refused(S=1, max_samples=2 ** 31)
    # the signal
    assert refused(amplitude=-1) and refused(amplitude=32768) and refused(sigma=-1) and refused(sigma=32768)
    # the configuration
    bad = A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS)
    bad.hop = 12
    assert refused(cfg=bad)
    k1 = A.make_cfg(n=1024, hop=256, freqs=(1500.0,))
    assert refused(cfg=k1, sync=[0], idle=[0])
    with pytest.raises(A.DemodError):
        A.make_tx_cfg(np.zeros(A.DEMOD_MAX_SYNC + 1, np.uint8))
    with pytest.raises(A.DemodError):
        A.tx_modulate_workspace_size(cfg, A.make_tx_cfg(**base), 0)


# ---- the reference modulator ---------------------------------------------------------

def pieces_equal_one_pull(c, S, sends, total, sizes):
    """Two transmitters, `sends` = {sample position: frames}: one pulls whole
    strides, the other pieces of `sizes` in turn; a send happens when its
    position is reached (positions are sums of pieces by construction)."""
    out = []
    for scheme in (None, sizes):
        tx, at, k, got = T.Tx(c, S), 0, 0, [[] for _ in range(S)]
        while at < total:
            if at in sends:
                assert (tx.send(sends[at])["status"] == T.OK).all()
            nxt = min([p for p in sends if p > at] + [total])
            m = min(c.stride if scheme is None else scheme[k % len(scheme)], nxt - at)
            k += 1
            for s, x in enumerate(tx.pull(m)):
                got[s].append(x)
            at += m
        out.append(([np.concatenate(g) for g in got], tx.state.copy()))
    return out


@pytest.mark.parametrize("K,fec", [(2, 0), (8, 1)])
def test_reference_pieces_equal_one_pull(lut, K, fec):
    """Pieces of 1, 7, 8, 9, n - 1, n, n + 1 and 2880 samples give the bytes of
    whole pulls, through a pull that ends mid-symbol in idle and is followed by
    a send, underflow into idle and a second send."""
    n = 64
    word = np.arange(8) % K
    c = T.make(tones(K), n, lut, word, h=1, kind=C.CRC16, fec=fec, max_len=4, gap=2, idle=(1, 0, 0), amplitude=9000,
               sigma=300, seed=5, max_frames=2, stride=2880)
    c.C = 2 * (T.frame_count(c, 4) + 2) + 3
    first = 2 * n + 17                       # mid-symbol, in idle
    second = first + (2 * (T.frame_count(c, 4) + 2) + 9) * n + 5    # after the queue ran dry
    sends = {first: [(1, b"\x01\x02\x03\x04"), (0, b""), (1, b"z")], second: [(0, b"abc"), (1, b"\xff")]}
    total = second + 4 * c.C * n
    (whole, st0), (cut, st1) = pieces_equal_one_pull(c, 2, sends, total, [1, 7, 8, 9, n - 1, n, n + 1, 2880])
    for s in range(2):
        assert whole[s].size == total and np.array_equal(whole[s], cut[s]), s
    assert st0.tobytes() == st1.tobytes()
    assert int(st0["accepted"].sum()) == 5 and st0["offset"][0] == total % n
    assert (st0["tail"] == st0["head"] + 1).all()         # idle, mid-symbol: the symbol in flight is consumed


def test_reference_phase_is_continuous(lut):
    """Without noise the phase advances by the symbol's increment at every
    sample, across symbol boundaries and from queued symbols into idle."""
    K, n = 4, 64
    c = T.make(tones(K), n, lut, [3, 0, 2], h=1, kind=C.CRC16, max_len=2, idle=(1, 2), amplitude=32767, sigma=0,
               max_frames=1, stride=8000)
    tx = T.Tx(c, 1)
    tx.send([(0, b"hi")])
    A_ = T.frame_count(c, 2)
    x = tx.pull((A_ + 4) * n)[0]
    sym = np.concatenate([T.frame_symbols(c, b"hi"), [T.idle_symbol(c, A_ + j) for j in range(4)]])
    ph = np.concatenate([np.zeros(1, np.uint64), np.cumsum(np.repeat(c.inc[sym], n))[:-1]]) & np.uint64(T.M32)
    want = (32767 * c.lut[(ph >> np.uint64(18)).astype(np.int64)] + 16384) >> 15
    assert np.array_equal(x, want.astype(np.int16))


# ---- the reference signal through the oracle detector and the frame references ----------

@pytest.mark.parametrize("fec", [0, 1])
@pytest.mark.parametrize("K", [2, 8])
def test_reference_loopback(O, lut, K, fec):
    """Amplitude 8000, sigma 400, hop = n / 4: scan -> check (or decode -> coded
    check) of the oracle detector's outputs returns every frame at R start, also
    with leading samples dropped. This fixes the inputs of the GPU loopback test
    as ones for which the reference alone returns all frames."""
    c, datas, N, total = T.loopback_case(K, fec, lut)
    n, hop = T.LOOP_N, T.LOOP_HOP
    R = n // hop
    tx = T.Tx(c, 1)
    lead = tx.pull([2880])[0], tx.pull([2880])[0]
    place = tx.send([(0, d) for d in datas])
    assert (place["status"] == T.OK).all() and place["start"][0] == -(-T.LOOP_LEAD // n)
    rest = [tx.pull([2880])[0] for _ in range((total - T.LOOP_LEAD) // 2880)]
    pcm = np.concatenate(list(lead) + rest)
    assert pcm.size == total
    for drop in (0, 3 * hop):
        sym, P = O.goertzel(pcm[drop:], tones(K), n, hop)
        got = X.one_shot(sym, P.astype(np.float32), R, c.sync, 0, N, c.h, c.kind, fec)
        assert [(w, b) for w, _, b in got] == [(R * int(p["start"]) - drop // hop, d) for p, d in zip(place, datas)]


# ---- the host sources under the sanitizers --------------------------------------------------

def test_standalone_program_under_sanitizers(tmp_path):
    """tests/native/tx_host_test.c with the host sources, built with
    -fsanitize=address,undefined and run as a program of its own."""
    csrc = os.path.join(ROOT, "audio-network_amd", "csrc")
    exe = str(tmp_path / "tx_host_test")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "native", "tx_host_test.c"), os.path.join(csrc, "demod_tx_frame.c"),
                    os.path.join(csrc, "demod_fec.c"), os.path.join(csrc, "demod_frame_check.c"),
                    os.path.join(csrc, "demod_frame.c"), "-lm", "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "300", "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "tx_host_test OK" in r.stdout
