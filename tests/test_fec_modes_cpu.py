"""The coded modes without a GPU (include/demod.h "punctured and interleaved"):
the map against tests/fec_modes_ref.py, the free distances of the puncturing
patterns by a trellis search, the encoder and the host decoder
demod_fec_frame_decode against the reference bit for bit, bursts with and
without the interleaver, every refusal, and the host sources in a standalone
program under AddressSanitizer and UBSan (tests/native/fec_modes_host_test.c).
"""
import ctypes
import heapq
import os
import subprocess

import numpy as np
import pytest

import fec_modes_ref as Z
import frames_check_ref as C
import frames_fec_ref as X

KINDS = (C.CRC16, C.CRC32)
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MAX_LEN = 40            # rows that hold every edge length of fec_modes_ref.edge_lengths


def test_exports_and_constants(A):
    lib = A.load_library()
    for name in ("demod_fec_air_index", "demod_fec_frame_symbols", "demod_fec_frame_encode",
                 "demod_fec_row_bytes", "demod_fec_frame_decode", "demod_fec_decode_workspace_size"):
        assert hasattr(lib, name), name
        assert name in A.header_exports()
    assert (A.DEMOD_FEC_CONV_K7, A.DEMOD_FEC_RATE_2_3, A.DEMOD_FEC_RATE_3_4, A.DEMOD_FEC_INTERLEAVE) == \
        (1, 0x10, 0x20, 0x40)
    assert A.DEMOD_FEC_IL_ROWS * A.DEMOD_FEC_IL_COLS == Z.BLOCK
    assert tuple(sorted(A.FEC_MODES)) == Z.MODES


# ---- 1. the map -----------------------------------------------------------------------

@pytest.mark.parametrize("fec", Z.MODES)
def test_map(A, fec):
    """demod_fec_air_index against the numpy map for m < 4096; a bijection
    between the kept bits and [0, Nt); the interleaver an involution; St(Nt(T))
    = T; and the library's symbol and row counts against the counted ones."""
    T = 2048
    want = Z.air_map(fec, T)
    got = np.array([A.fec_air_index(fec, m) for m in range(2 * T)], np.int64)
    assert np.array_equal(got, want)
    for t in (0, 1, 2, 3, 5, 6, 7, 127, 128, 129, 383, 384, 385, 2048):
        kept = want[:2 * t][want[:2 * t] >= 0]
        Nt = Z.kept_bits(fec, t)
        assert kept.size == Nt and np.unique(kept).size == Nt
        code = np.array([Z.interleave(fec, int(a)) for a in kept], np.int64)   # back: the same function
        assert np.array_equal(code, np.arange(Nt))                             # ranks in step order
        assert Z.steps_within(fec, Nt) == t or (t == 0 and Z.steps_within(fec, 0) == 0)
    if fec & Z.INTERLEAVE:
        i = np.arange(4096)
        a = np.array([Z.interleave(fec, int(v)) for v in i])
        assert np.array_equal(np.array([Z.interleave(fec, int(v)) for v in a]), i)
        assert np.array_equal(a // Z.BLOCK, i // Z.BLOCK) and not np.array_equal(a, i)
    for h in (1, 2):
        for kind in KINDS:
            for bits in (1, 2, 3, 4):
                for length in (0, 1, 5, 6, 38, 255):
                    assert A.fec_frame_symbols(length, h, kind, bits, fec) == \
                        Z.span(length, bits, h, kind, fec)
                for N in range(86, 400, 7):
                    shape = Z.row_shape(N, bits, h, kind, fec)
                    St = Z.steps_within(fec, N * bits // Z.BLOCK * Z.BLOCK if fec & Z.INTERLEAVE else N * bits)
                    if St < 8 * h + X.DEPTH:
                        with pytest.raises(A.DemodError):
                            A.fec_row_bytes(N, bits, h, fec)
                    else:
                        assert A.fec_row_bytes(N, bits, h, fec) == (St - 6) // 8
                        assert A.fec_row_steps(N * bits, fec) == St
                        assert shape is None or shape[1] == (St - 6) // 8


def test_old_functions_are_mode_1(A):
    rng = np.random.default_rng(1)
    cfg = A.make_cfg(n=1024, hop=256, freqs=tuple(1500.0 + 375.0 * i for i in range(8)))
    for h in (1, 2):
        for kind in KINDS:
            for length in (0, 1, 6, 7, 33):
                data = rng.integers(0, 256, length).astype(np.uint8).tobytes()
                assert A.fec_frame_encode(data, h, kind, 1) == A.coded_frame_encode(data, h, kind)
                for bits in (1, 2, 3, 4):
                    assert A.fec_frame_symbols(length, h, kind, bits, 1) == A.coded_frame_symbols(length, h, kind, bits)
            for n_soft in (2 * (8 * h + 64), 2 * (8 * h + 64) + 1, 700, 701):
                soft = rng.integers(-127, 128, n_soft).astype(np.int8)
                assert A.fec_frame_decode(soft, h, kind, 1) == A.coded_frame_decode(soft, h, kind)
        for N in (160, 161, 400):
            for bits in (1, 2, 3, 4):
                assert A.fec_row_bytes(N, bits, h, 1) == A.coded_row_bytes(N, bits, h)
    for S, cap, N in ((1, 8, 200), (3, 70, 333), (1024, 32, 90)):
        assert A.fec_decode_workspace_size(cfg, S, cap, N, 1) == A.frames_decode_workspace_size(cfg, S, cap, N)
    # a punctured row has up to 3/4 C steps: the workspace grows with St
    for fec in Z.MODES:
        St = Z.row_shape(333, 3, 1, C.CRC16, fec)[0]
        assert A.fec_decode_workspace_size(cfg, 3, 70, 333, fec) == 3 * 70 * St * 8


# ---- 2. free distances ------------------------------------------------------------------

def free_distance(fec):
    """The least weight of a path that leaves the all-zero path and rejoins it,
    over every step phase it can leave at: Dijkstra over (phase, state), the
    weight of a branch the ones among its kept output bits."""
    pat = Z.pattern(fec)
    P = len(pat)

    def branch(phase, state, u):
        reg = ((state << 1) | u) & 0x7F
        out = (X.parity(reg & X.G0), X.parity(reg & X.G1))
        return reg & 63, sum(out[v] for v in pat[phase])
    best = None
    for start in range(P):
        s, w = branch(start, 0, 1)
        dist = {((start + 1) % P, s): w}
        heap = [(w, (start + 1) % P, s)]
        while heap:
            w, ph, s = heapq.heappop(heap)
            if dist.get((ph, s), 1 << 30) < w:
                continue
            if s == 0:
                best = w if best is None else min(best, w)
                break
            for u in (0, 1):
                s2, dw = branch(ph, s, u)
                key = ((ph + 1) % P, s2)
                if w + dw < dist.get(key, 1 << 30):
                    dist[key] = w + dw
                    heapq.heappush(heap, (w + dw, key[0], s2))
    return best


def test_free_distances():
    assert [free_distance(f) for f in (0x01, 0x11, 0x21)] == [10, 6, 5]


# ---- 3. and 4. encoder and host decoder ----------------------------------------------------

def rows_for(fec, h, kind):
    """N (at 1 bit a symbol) of rows that hold MAX_LEN data bytes, a few bits more."""
    return Z.symbols_for(MAX_LEN, 1, h, kind, fec) + 5


@pytest.mark.parametrize("fec", Z.MODES)
def test_encoder(A, fec):
    """Byte for byte at the edge lengths, pad bits 0; cap one short is refused."""
    rng = np.random.default_rng(fec)
    for h in (1, 2):
        for kind in KINDS:
            max_len = Z.row_shape(rows_for(fec, h, kind), 1, h, kind, fec)[2]
            for length in Z.edge_lengths(max_len, h, kind, fec):
                data = rng.integers(0, 256, length).astype(np.uint8).tobytes()
                want = Z.encode(data, h, kind, fec)
                assert A.fec_frame_encode(data, h, kind, fec) == want, (h, kind, length)
                assert A.fec_frame_encode(data, h, kind, fec, cap=len(want)) == want
                with pytest.raises(A.DemodError) as e:
                    A.fec_frame_encode(data, h, kind, fec, cap=len(want) - 1)
                assert e.value.code == A.DEMOD_BUFFER_TOO_SMALL


def same_decode(A, soft, h, kind, fec, what):
    got = A.fec_frame_decode(soft, h, kind, fec)
    want = Z.decode(soft, h, kind, fec)
    assert got[0] == want[0], what
    assert tuple(got[1][f] for f in X.DECODE_DTYPE.names) == tuple(int(want[1][f]) for f in X.DECODE_DTYPE.names), what
    return got


@pytest.mark.parametrize("fec", Z.MODES)
def test_host_decoder(A, fec):
    """demod_fec_frame_decode equal to the reference (the air soft values
    re-ordered into a rate-1/2 trellis array, through frames_fec_ref.decode):
    the edge-length frames with 4 inverted values and random values behind
    them, all-zero soft values, a header of max_len + 1, and the minimal row
    (one block interleaved: N = 86 at 3 bits a symbol)."""
    rng = np.random.default_rng(100 + fec)
    for h in (1, 2):
        for kind in KINDS:
            Cc = rows_for(fec, h, kind)
            St, Bd, max_len = Z.row_shape(Cc, 1, h, kind, fec)
            clean = 0
            for length in Z.edge_lengths(max_len, h, kind, fec):
                frame = C.encode(rng.integers(0, 256, length).astype(np.uint8).tobytes(), h, kind)
                air = Z.encode_air(frame, X.steps(length, h, kind), fec)
                air[rng.choice(air.size, 4, replace=False)] ^= 1
                soft = X.hard_soft(air, rng, Cc - air.size)
                got = same_decode(A, soft, h, kind, fec, (h, kind, length))
                clean += got[0] == frame
            assert clean >= 1
            same_decode(A, np.zeros(Cc, np.int8), h, kind, fec, "zeros")
            info = (max_len + 1).to_bytes(h, "big") + rng.integers(0, 256, Bd).astype(np.uint8).tobytes()
            soft = X.hard_soft(Z.encode_air(info, St, fec))[:Cc]
            soft = np.concatenate([soft, np.zeros(Cc - soft.size, np.int8)])
            got = same_decode(A, soft, h, kind, fec, "max_len + 1")
            assert got[1]["status"] == A.DEMOD_DECODE_BAD_LENGTH and got[1]["length"] == max_len + 1
    # the minimal rows
    for h in (1, 2):
        t0 = 8 * h + X.DEPTH
        Cmin = Z.BLOCK if fec & Z.INTERLEAVE and Z.steps_within(fec, Z.BLOCK) >= t0 else None
        if Cmin is None:
            Cmin = next(c for c in range(1, 4096) if Z.row_shape(c, 1, h, C.CRC16, fec) is not None)
        for Cc in (Cmin, Cmin + 1, Cmin + 2):
            soft = rng.integers(-127, 128, Cc).astype(np.int8)
            same_decode(A, soft, h, C.CRC16, fec, ("minimal", Cc))
        with pytest.raises(A.DemodError):
            A.fec_frame_decode(np.zeros(Cmin - 1, np.int8), h, C.CRC16, fec)
    if fec == 0x41:
        assert Z.row_shape(86, 3, 1, C.CRC16, fec) == (128, 15, 12) and Z.row_shape(85, 3, 1, C.CRC16, fec) is None


# ---- 5. bursts -------------------------------------------------------------------------------

BURST_H, BURST_KIND, BURST_LEN = 2, C.CRC16, 20        # an information block of 24 bytes


def burst_losses(A, fec, width, erase):
    """The offsets at which a burst of `width` consecutive air bits (inverted,
    or erased) loses the frame, and the offsets tried: every one in the frame."""
    rng = np.random.default_rng(24)
    frame = C.encode(rng.integers(0, 256, BURST_LEN).astype(np.uint8).tobytes(), BURST_H, BURST_KIND)
    assert len(frame) == 24
    air = Z.encode_air(frame, X.steps(BURST_LEN, BURST_H, BURST_KIND), fec)
    clean = X.hard_soft(air)
    assert A.fec_frame_decode(clean, BURST_H, BURST_KIND, fec)[0] == frame
    lost = []
    offsets = range(air.size - width + 1)
    for at in offsets:
        soft = clean.copy()
        soft[at:at + width] = 0 if erase else -soft[at:at + width]
        row, dec = A.fec_frame_decode(soft, BURST_H, BURST_KIND, fec)
        if row != frame or dec["status"] != A.DEMOD_DECODE_OK:
            lost.append(at)
    return lost, len(offsets)


@pytest.mark.parametrize("rate,inverted", [(0, 12), (Z.RATE_2_3, 12), (Z.RATE_3_4, 3)])
def test_bursts(A, rate, inverted):
    """A 24-byte information block, +-127 soft values, a burst at every
    offset: the interleaved mode recovers every burst of `inverted` inverted
    bits and of 32 erased ones, the plain order of the same rate loses at
    least one of each."""
    plain, spread = Z.CONV_K7 | rate, Z.CONV_K7 | rate | Z.INTERLEAVE
    for width, erase in ((inverted, False), (32, True)):
        lost, tried = burst_losses(A, spread, width, erase)
        print(f"fec {spread:#x} {'erased' if erase else 'inverted'} {width}: lost {len(lost)} of {tried}")
        lost_plain, tried_plain = burst_losses(A, plain, width, erase)
        print(f"fec {plain:#x} {'erased' if erase else 'inverted'} {width}: lost {len(lost_plain)} of {tried_plain}")
        assert not lost, (hex(spread), width, erase, lost[:8])
        assert lost_plain, (hex(plain), width, erase)


# ---- 6. refusals -----------------------------------------------------------------------------

def test_refusals(A):
    """fec of 2, 0x10, 0x31 and 0x81, 0x41 with K = 3, and an interleaved row
    shorter than one block: every host function, demod_rx_sizes,
    demod_tx_sizes and the mirror."""
    lib = A.load_library()
    soft = np.zeros(512, np.int8)
    row = np.zeros(64, np.uint8)
    out = (ctypes.c_uint8 * 128)()
    dec = A.DemodFrameDecode()
    cfg2 = A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS)
    cfg3 = A.make_cfg(n=1024, hop=256, freqs=(1500.0, 2250.0, 3000.0))
    word = [0, 1, 1, 0, 1]
    rx_base = dict(sync=word, max_errors=0, frame_symbols=600, len_bytes=1, crc=C.CRC16, max_frames=4,
                   ring_windows=2 * 605 * 4)
    tx_base = dict(sync=word, len_bytes=1, crc=C.CRC16, max_len=16, ring_symbols=4096)
    for fec in Z.MODES:                                   # the cases below differ from legal calls in fec alone
        assert A.rx_sizes(cfg2, A.make_rx_cfg(fec=fec, **rx_base), 2)["decode_work_bytes"] == \
            A.fec_decode_workspace_size(cfg2, 2, 4, 600, fec)
        assert A.tx_sizes(cfg2, A.make_tx_cfg(fec=fec, **tx_base), 2)["max_symbols"] == \
            5 + Z.span(16, 1, 1, C.CRC16, fec)
    for fec in Z.BAD_MODES:
        assert lib.demod_fec_air_index(fec, 0) == A.DEMOD_BAD_ARG
        assert lib.demod_fec_frame_symbols(0, 1, C.CRC16, 1, fec) == A.DEMOD_BAD_ARG
        assert lib.demod_fec_frame_encode(None, 0, 1, C.CRC16, fec, out, 128) == A.DEMOD_BAD_ARG
        assert lib.demod_fec_row_bytes(512, 1, 1, fec) == A.DEMOD_BAD_ARG
        assert lib.demod_fec_frame_decode(soft.ctypes.data, 512, 1, C.CRC16, fec, row.ctypes.data, 64,
                                          ctypes.byref(dec)) == A.DEMOD_BAD_ARG
        assert lib.demod_fec_decode_workspace_size(ctypes.byref(cfg2), 1, 4, 600, fec) == 0
        with pytest.raises(A.DemodError):
            A.rx_sizes(cfg2, A.make_rx_cfg(fec=fec, **rx_base), 2)
        with pytest.raises(A.DemodError):
            A.tx_sizes(cfg2, A.make_tx_cfg(fec=fec, **tx_base), 2)
        with pytest.raises(A.DemodError):
            A.tx_frame_symbols(A.make_tx_cfg(fec=fec, **tx_base), 2, b"ab")
        for call in (lambda: A.fec_air_index(fec, 0), lambda: A.fec_frame_symbols(0, 1, C.CRC16, 1, fec),
                     lambda: A.fec_frame_encode(b"", 1, C.CRC16, fec), lambda: A.fec_row_bytes(512, 1, 1, fec),
                     lambda: A.fec_frame_decode(soft, 1, C.CRC16, fec), lambda: A.fec_row_steps(512, fec),
                     lambda: A.fec_decode_workspace_size(cfg2, 1, 4, 600, fec)):
            with pytest.raises(A.DemodError) as e:
                call()
            assert e.value.code == A.DEMOD_BAD_ARG
    # K = 3: a coded bit would ask for a tone that does not exist
    with pytest.raises(A.DemodError):
        A.rx_sizes(cfg3, A.make_rx_cfg(fec=0x41, **rx_base), 2)
    with pytest.raises(A.DemodError):
        A.tx_sizes(cfg3, A.make_tx_cfg(fec=0x41, **tx_base), 2)
    with pytest.raises(A.DemodError):
        A.tx_frame_symbols(A.make_tx_cfg(fec=0x41, **tx_base), 3, b"ab")
    with pytest.raises(A.DemodError):
        A.fec_decode_workspace_size(cfg3, 1, 4, 600, 0x41)
    # an interleaved row shorter than one block
    assert lib.demod_fec_row_bytes(255, 1, 1, 0x41) == A.DEMOD_BAD_ARG
    assert lib.demod_fec_row_bytes(85, 3, 1, 0x41) == A.DEMOD_BAD_ARG and lib.demod_fec_row_bytes(86, 3, 1, 0x41) == 15
    assert lib.demod_fec_frame_decode(soft.ctypes.data, 255, 1, C.CRC16, 0x41, row.ctypes.data, 64,
                                      ctypes.byref(dec)) == A.DEMOD_BAD_ARG
    with pytest.raises(A.DemodError):
        A.rx_sizes(cfg2, A.make_rx_cfg(fec=0x41, **dict(rx_base, frame_symbols=255)), 2)
    A.rx_sizes(cfg2, A.make_rx_cfg(fec=0x41, **dict(rx_base, frame_symbols=256)), 2)
    # the mirror's device entries judge fec before any tensor
    d = object.__new__(A.Demodulator)
    d._lib, d.cfg, d._h = lib, cfg2, None
    for fec in Z.BAD_MODES + (0,):
        with pytest.raises(A.DemodError) as e:
            d.frames_decode_async(None, None, 100, None, None, 1, 4, 5, 600, 1, C.CRC16, None, None, None, fec=fec)
        assert "fec" in str(e.value)
        with pytest.raises(A.DemodError) as e:
            d.frames_check_coded_async(None, None, None, 1, 4, 5, 600, 1, C.CRC16, None, None, None, None, fec=fec)
        assert "fec" in str(e.value)
        with pytest.raises(A.DemodError) as e:
            d.frames_coded(np.zeros(8192, np.int16), word, frame_symbols=600, fec=fec)
        assert "fec" in str(e.value)
        if fec:
            with pytest.raises(A.DemodError) as e:
                d.rx_collect_async(None, None, None, None, None, None, None, 1, 4, 5, 600, 1, C.CRC16, fec, None,
                                   None, None, None)
            assert "fec" in str(e.value)
    with pytest.raises(A.DemodError) as e:                # shorter than one block: the look-ahead cannot fit
        d.frames_decode_async(None, None, 100, None, None, 1, 4, 5, 255, 1, C.CRC16, None, None, None, fec=0x41)
    assert "look-ahead" in str(e.value)


# ---- 7. the host sources under sanitizers -------------------------------------------------------

def test_standalone_program_under_sanitizers(tmp_path):
    """tests/native/fec_modes_host_test.c with the host sources, built with
    -fsanitize=address,undefined and run as a program of its own."""
    csrc = os.path.join(ROOT, "audio-network_amd", "csrc")
    exe = str(tmp_path / "fec_modes_host_test")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "native", "fec_modes_host_test.c"), os.path.join(csrc, "demod_fec.c"),
                    os.path.join(csrc, "demod_tx_frame.c"), os.path.join(csrc, "demod_frame_check.c"),
                    os.path.join(csrc, "demod_frame.c"), "-lm", "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "fec_modes_host_test OK" in r.stdout
