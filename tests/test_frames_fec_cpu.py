"""Coded frames without a GPU: the ABI (exports, struct layout), the encoder,
demod_soft_bits and the host decoder demod_coded_frame_decode against
tests/frames_fec_ref.py bit for bit, 2000 frames with 4 inverted soft values
each, the round trip through demod_unpack_symbols, the Python mirror's
refusals, and the host sources in a standalone program under AddressSanitizer
and UBSan (tests/native/fec_host_test.c)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import frames_check_ref as C
import frames_fec_ref as X

KINDS = (C.CRC16, C.CRC32)
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_exports_and_structs(A):
    lib = A.load_library()
    for name in ("demod_coded_frame_steps", "demod_coded_frame_symbols", "demod_coded_frame_encode",
                 "demod_coded_row_bytes", "demod_soft_bits", "demod_coded_frame_decode",
                 "demod_frames_decode_workspace_size", "demod_frames_decode_async",
                 "demod_frames_check_coded_async", "demod_frames_coded"):
        assert hasattr(lib, name), name
        assert name in A.header_exports()
    for name in ("frames_decode_async", "frames_check_coded_async", "frames_coded"):
        assert callable(getattr(A.Demodulator, name))
    T = A.DemodFrameDecode
    assert ctypes.sizeof(T) == 16
    assert (T.length.offset, T.metric.offset, T.status.offset, T.steps.offset) == (0, 4, 8, 12)
    assert A.FRAME_DECODE_DTYPE == X.DECODE_DTYPE
    assert (A.DEMOD_FEC_CONV_K7, A.DEMOD_FEC_DEPTH) == (X.CONV_K7, X.DEPTH) == (1, 64)
    assert (A.DEMOD_DECODE_OK, A.DEMOD_DECODE_BAD_LENGTH) == (X.OK, X.BAD_LENGTH) == (0, 1)
    assert lib.demod_frames_decode_async(None, None, None, 4, None, None, 1, 1, 1, 144, 1, 1, 1, None, None,
                                         None, 0, None) == A.DEMOD_BAD_ARG
    assert lib.demod_frames_check_coded_async(None, None, None, None, 1, 1, 1, 144, 1, 1, 1, None, None, None,
                                              None, None) == A.DEMOD_BAD_ARG
    res, summ = A.DemodFramesResult(), A.DemodFramesCheckResult()
    assert lib.demod_frames_coded(None, None, 4, None, 0, 0, 144, 1, 1, 1, None, None, None, 1,
                                  ctypes.byref(res), ctypes.byref(summ)) == A.DEMOD_BAD_ARG


def test_workspace_size(A):
    """waves x St x 8, the waves capped as the check caps them; 0 for what is refused."""
    cfg = A.make_cfg(n=1024, hop=256, freqs=tuple(1500.0 + 375.0 * i for i in range(8)))
    assert A.frames_decode_workspace_size(cfg, 1, 1, 48) == 72 * 8
    assert A.frames_decode_workspace_size(cfg, 1, 5, 49) == 5 * 73 * 8
    assert A.frames_decode_workspace_size(cfg, 1, 10 ** 6, 48) == 16384 * 72 * 8
    assert A.frames_decode_workspace_size(cfg, 1024, 32, 48) == 1024 * 16 * 72 * 8
    assert A.frames_decode_workspace_size(cfg, 3, 10 ** 5, 48) == 3 * 5461 * 72 * 8
    assert A.frames_decode_workspace_size(cfg, 65536, 7, 48) == 65536 * 72 * 8
    five = A.make_cfg(n=1024, hop=256, freqs=tuple(1500.0 + 375.0 * i for i in range(5)))
    for args in ((cfg, 0, 1, 48), (cfg, 65537, 1, 48), (cfg, 1, 0, 48), (cfg, 2 ** 15, 2 ** 16, 48),
                 (cfg, 1, 1, 0), (cfg, 1, 1, 2 ** 31), (five, 1, 1, 48), (cfg, -1, 1, 48)):
        with pytest.raises(A.DemodError):
            A.frames_decode_workspace_size(*args)


def test_workspace_size_across_the_wave_cap(A):
    """include/demod.h's description as a closed form, n_groups min(max_frames,
    max(16384 / n_groups, 1)) St 8, on both sides of the cap of 16384 waves:
    where 16384 / n_groups is below max_frames, exactly 1, and 0; at 1 and 4
    bits a symbol."""
    pairs = [(4096, 5), (5461, 4), (8193, 3), (16384, 2), (16385, 3), (65536, 2),
             (1, 1), (1, 16384), (1, 16385), (16383, 2), (65536, 1)]
    for K, N in ((2, 145), (16, 36), (16, 39)):
        bits = K.bit_length() - 1
        cfg = A.make_cfg(n=1024, hop=256, freqs=tuple(1500.0 + 375.0 * i for i in range(K)))
        St = N * bits // 2
        for S, max_frames in pairs:
            want = S * min(max_frames, max(16384 // S, 1)) * St * 8
            assert A.frames_decode_workspace_size(cfg, S, max_frames, N) == want, (K, N, S, max_frames)
    assert A.frames_decode_workspace_size(cfg, 65536, 2, 36) == 65536 * 72 * 8


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h", [1, 2])
def test_encoder(A, h, kind):
    """Byte for byte against the reference, T and Sc, and every refusal."""
    rng = np.random.default_rng(10 * h + kind)
    c = C.CRC_BYTES[kind]
    for n in [0, 1, 2, 7 - c, 8 - c, 9, 40, 255, 256, 4096, 4097] + rng.integers(0, 300, 12).tolist():
        d = rng.integers(0, 256, n).astype(np.uint8).tobytes()
        want = X.encode(d, h, kind)
        if want is None:
            for fn in (lambda: A.coded_frame_encode(d, h, kind), lambda: A.coded_frame_steps(n, h, kind),
                       lambda: A.coded_frame_symbols(n, h, kind, 1)):
                with pytest.raises(A.DemodError) as e:
                    fn()
                assert e.value.code == A.DEMOD_FRAME_TOO_LARGE
            continue
        T = X.steps(n, h, kind)
        assert A.coded_frame_steps(n, h, kind) == T == max(8 * (h + n + c) + 6, 8 * h + 64)
        got = A.coded_frame_encode(d, h, kind)
        assert got == want and len(got) == (2 * T + 7) // 8
        assert A.coded_frame_encode(d, h, kind, cap=len(want)) == want
        with pytest.raises(A.DemodError) as e:
            A.coded_frame_encode(d, h, kind, cap=len(want) - 1)
        assert e.value.code == A.DEMOD_BUFFER_TOO_SMALL
        for bits in (1, 2, 3, 4):
            assert A.coded_frame_symbols(n, h, kind, bits) == X.coded_symbols(n, h, kind, bits) == -(-2 * T // bits)
    for kw in (dict(len_bytes=0), dict(len_bytes=3), dict(crc=0), dict(crc=3)):
        kw = dict(dict(len_bytes=h, crc=kind), **kw)
        with pytest.raises(A.DemodError) as e:
            A.coded_frame_encode(b"abc", **kw)
        assert e.value.code == A.DEMOD_BAD_ARG
        with pytest.raises(A.DemodError):
            A.coded_frame_steps(3, **kw)
    for bits in (0, 5, -1):
        with pytest.raises(A.DemodError) as e:
            A.coded_frame_symbols(3, h, kind, bits)
        assert e.value.code == A.DEMOD_BAD_ARG
    lib = A.load_library()
    out = (ctypes.c_uint8 * 64)()
    assert lib.demod_coded_frame_encode(None, 3, h, kind, out, 64) == A.DEMOD_BAD_ARG
    assert lib.demod_coded_frame_encode(None, 0, h, kind, None, 64) == A.DEMOD_BAD_ARG
    assert lib.demod_coded_frame_encode(None, 0, h, kind, out, 64) == (2 * (8 * h + 64) + 7) // 8


def test_row_bytes(A):
    for bits in (1, 2, 3, 4):
        for h in (1, 2):
            for N in (0, 1, 47, 48, 49, 72, 80, 143, 144, 145, 159, 160, 161, 1000, 33000):
                shape = X.row_shape(N, bits, h, C.CRC16)
                if N * bits // 2 < 8 * h + 64:
                    assert shape is None
                    with pytest.raises(A.DemodError):
                        A.coded_row_bytes(N, bits, h)
                else:
                    assert A.coded_row_bytes(N, bits, h) == (N * bits // 2 - 6) // 8
    for args in ((144, 0, 1), (144, 5, 1), (144, 1, 0), (144, 1, 3), (2 ** 31, 1, 1), (-1, 1, 1)):
        with pytest.raises(A.DemodError):
            A.coded_row_bytes(*args)


@pytest.mark.parametrize("K", [2, 4, 8, 16])
def test_soft_bits(A, K):
    """Random, equal, zero, negative, NaN and Inf powers, ties and values that
    round at .5: the library's double expression is numpy's, value for value."""
    rng = np.random.default_rng(K)
    P = np.concatenate([
        rng.integers(0, 3000, (300, K)).astype(np.float32),
        rng.normal(0.0, 1.0, (100, K)).astype(np.float32),
        (rng.random((100, K)) * 1e-38).astype(np.float32),            # subnormal sums
        (rng.random((50, K)) * 3e38).astype(np.float32),              # the float sum would overflow
        np.full((1, K), 7.0, np.float32), np.zeros((1, K), np.float32), -np.ones((1, K), np.float32),
        np.full((1, K), np.nan, np.float32), np.full((1, K), np.inf, np.float32),
        np.full((1, K), -np.inf, np.float32)])
    special = rng.integers(0, 3000, (60, K)).astype(np.float32)
    for i, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -5.0, 3.4e38)):
        for j in range(10):
            special[10 * i + j, rng.integers(0, K, 1 + j % 2)] = v
    x = np.arange(127, dtype=np.float32)                              # 127 d / s = x + .5 exactly: ties to even
    half = np.repeat((np.float32(126.5) - x)[:, None], K, axis=1)     # s = 254, d = 2 x + 1
    half[:, 0] = np.float32(127.5) + x
    P = np.concatenate([P, special, half])
    ref = X.soft_bits(P)
    assert np.abs(ref.astype(np.int32)).max() == 127 and (ref == 0).any()
    for w in range(len(P)):
        got = A.soft_bits(P[w])
        assert got.dtype == np.int8 and np.array_equal(got, ref[w]), (w, P[w], got, ref[w])
    # the strictly-greater rule: a NaN in the first tone of a class stays, elsewhere it is skipped
    first = np.ones(K, np.float32)
    first[0] = np.nan
    assert A.soft_bits(first)[0] == 0 == ref.dtype.type(X.soft_bits(first[None])[0, 0])
    if K > 2:
        later = np.arange(1, K + 1, dtype=np.float32)
        later[1] = np.nan
        assert np.array_equal(A.soft_bits(later), X.soft_bits(later[None])[0]) and A.soft_bits(later)[0] != 0
    for bad in (np.ones(1), np.ones(3), np.ones(5), np.ones(32), np.ones(0)):
        with pytest.raises(A.DemodError):
            A.soft_bits(bad)


def both(A, soft, h, kind):
    """The library's and the reference's decode of one row; asserted equal."""
    got = A.coded_frame_decode(soft, h, kind)
    want = X.decode(soft, h, kind)
    assert got[0] == want[0] and tuple(got[1][f] for f in X.DECODE_DTYPE.names) == tuple(want[1].tolist())
    return got


def frame_soft(rng, data, h, kind, n_soft, flips=4):
    """+-127 soft values of the coded frame, `flips` of them inverted, random values behind."""
    T = X.steps(len(data), h, kind)
    coded = X.encode_bits(C.encode(data, h, kind), T)[:n_soft]
    q = X.hard_soft(coded, rng, n_soft - coded.size)
    at = rng.choice(coded.size, flips, replace=False)
    q[at] = -q[at]
    return q


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h", [1, 2])
def test_decoder_edges(A, h, kind):
    """Lengths 0, 1, either side of 8 n + 6 = 8 h + 64, max_len and max_len +
    1, a header of all ones, all-zero soft values (every comparison ties), an
    odd C and the minimal row St = 8 h + 64."""
    rng = np.random.default_rng(100 * h + kind)
    c, t0 = C.CRC_BYTES[kind], 8 * h + 64
    for n_soft in (2 * t0, 2 * t0 + 1, 2 * t0 + 2, 2 * (8 * (h + 24 + c) + 6), 2 * (8 * (h + 24 + c) + 6) + 25):
        St, Bd, max_len = X.row_shape(1, n_soft, h, kind)
        assert St == n_soft // 2 and (n_soft > 2 * t0 or St == t0)
        for n in sorted({0, 1, 7 - c, 8 - c, max_len, max_len + 1}):
            data = rng.integers(0, 256, n).astype(np.uint8).tobytes()
            written, dec = both(A, frame_soft(rng, data, h, kind, n_soft, 4 if n <= max_len else 0), h, kind)
            if n <= max_len:
                assert written == C.encode(data, h, kind)
                assert dec == dict(length=n, metric=127 * (2 * X.steps(n, h, kind) - 8), status=X.OK,
                                   steps=X.steps(n, h, kind))
            else:
                assert written == n.to_bytes(h, "big")
                assert dec == dict(length=n, metric=0, status=X.BAD_LENGTH, steps=0)
        ones = X.hard_soft(X.encode_bits(b"\xff" * h, t0), rng, n_soft - 2 * t0)
        written, dec = both(A, ones, h, kind)
        assert written == b"\xff" * h and dec == dict(length=256 ** h - 1, metric=0, status=X.BAD_LENGTH, steps=0)
        written, dec = both(A, np.zeros(n_soft, np.int8), h, kind)
        assert written == bytes(h + c) and dec == dict(length=0, metric=0, status=X.OK, steps=t0)
        for _ in range(4):
            both(A, rng.integers(-127, 128, n_soft).astype(np.int8), h, kind)
            both(A, rng.integers(-2, 3, n_soft).astype(np.int8), h, kind)          # many ties
        with pytest.raises(A.DemodError) as e:
            A.coded_frame_decode(np.zeros(n_soft, np.int8), h, kind, cap=Bd - 1)
        assert e.value.code == A.DEMOD_BUFFER_TOO_SMALL
    for n_soft in (0, 1, 2 * t0 - 1, 2 * (8 * (h + 4097 + c) + 6)):
        with pytest.raises(A.DemodError) as e:
            A.coded_frame_decode(np.zeros(n_soft, np.int8), h, kind, cap=8192)
        assert e.value.code == A.DEMOD_BAD_ARG
    for kw in (dict(len_bytes=0), dict(len_bytes=3), dict(crc=0), dict(crc=3)):
        with pytest.raises(A.DemodError):
            A.coded_frame_decode(np.zeros(400, np.int8), **dict(dict(len_bytes=h, crc=kind), **kw))


def test_longest_row(A):
    """max_len 4096: 32822 steps through the library's decoder."""
    h, kind = 2, C.CRC32
    rng = np.random.default_rng(4096)
    data = rng.integers(0, 256, 4096).astype(np.uint8).tobytes()
    T = X.steps(4096, h, kind)
    q = frame_soft(rng, data, h, kind, 2 * T + 3, flips=4)
    written, dec = A.coded_frame_decode(q, h, kind)
    assert written == C.encode(data, h, kind) and dec["steps"] == T == 32822 and dec["status"] == X.OK


def test_four_flips_always_decode(A):
    """Any 4 inverted values of a +-127 frame, random values behind it: 2000
    seeded cases through the library's decoder, 0 failures allowed (every 20th
    also through the reference, which must agree bit for bit). Half the cases
    cluster the 4 inside 14 coded bits, half spread them over the header's
    first 2 (8 h + 64) coded bits or the whole frame."""
    rng = np.random.default_rng(2000)
    failures = []
    for case in range(2000):
        h, kind = int(rng.integers(1, 3)), KINDS[int(rng.integers(0, 2))]
        data = rng.integers(0, 256, int(rng.integers(0, 41))).astype(np.uint8).tobytes()
        T = X.steps(len(data), h, kind)
        q = X.hard_soft(X.encode_bits(C.encode(data, h, kind), T), rng, int(rng.integers(0, 300)))
        if case % 2:
            lo = int(rng.integers(0, 2 * T - 14))
            at = lo + rng.choice(14, 4, replace=False)
        else:
            at = rng.choice(2 * (8 * h + 64) if case % 4 else 2 * T, 4, replace=False)
        q[at] = -q[at]
        written, dec = both(A, q, h, kind) if case % 20 == 0 else A.coded_frame_decode(q, h, kind)
        if written != C.encode(data, h, kind) or dec["status"] != X.OK or dec["steps"] != T:
            failures.append(case)
    assert not failures, failures[:10]


@pytest.mark.parametrize("bits", [1, 3, 4])
def test_round_trip_through_symbols(A, bits):
    """coded bytes -> demod_unpack_symbols -> one loud tone per symbol ->
    demod_soft_bits -> decoder: the frame comes back; Sc symbols hold it."""
    rng = np.random.default_rng(bits)
    K = 1 << bits
    for h in (1, 2):
        for kind in KINDS:
            for n in (0, 5, 33):
                data = rng.integers(0, 256, n).astype(np.uint8).tobytes()
                coded = A.coded_frame_encode(data, h, kind)
                Sc = A.coded_frame_symbols(n, h, kind, bits)
                pad = coded + b"\0" if Sc * bits > 8 * len(coded) else coded
                sym = A.unpack_symbols(pad, Sc, bits)
                assert np.array_equal(sym, C.unpack(coded, Sc, bits))
                N = Sc + 7
                row = np.concatenate([sym, rng.integers(0, K, N - Sc).astype(np.uint8)])
                P = rng.integers(1, 300, (N, K)).astype(np.float32)
                P[np.arange(N), row] = 2000.0
                soft = np.concatenate([A.soft_bits(P[j]) for j in range(N)])
                assert np.array_equal(soft, X.soft_bits(P).reshape(-1))
                hard = (soft < 0).astype(np.uint8).reshape(N, bits)
                assert np.array_equal((hard << np.arange(bits - 1, -1, -1)).sum(axis=1), row)
                written, dec = both(A, soft, h, kind)
                assert written == C.encode(data, h, kind) and dec["steps"] == X.steps(n, h, kind)
                assert A.coded_row_bytes(N, bits, h) == X.row_shape(N, bits, h, kind)[1]


def test_python_mirror_refuses_before_the_library(A):
    """No device here: every path of Demodulator.frames_decode_async and
    frames_check_coded_async ends in the mirror's own checks (the C refusals
    are tests/test_gpu_frames_fec.py's)."""
    torch = pytest.importorskip("torch")
    d = object.__new__(A.Demodulator)
    d._lib, d.cfg, d._h = A.load_library(), A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS), None
    N, cap, W = 200, 4, 1000

    def t(nbytes, dtype=torch.uint8):
        return torch.zeros(nbytes, dtype=dtype)

    def call(fn="frames_decode_async", **kw):
        if fn == "frames_decode_async":
            a = dict(d_hits=t(cap * 16), d_mag=t(W * 2, torch.float32), n_windows=W, d_first=None,
                     d_results=t(560), n_groups=1, max_frames=cap, sync_len=8, frame_symbols=N, len_bytes=1,
                     crc=A.DEMOD_CRC16_CCITT_FALSE, d_rows=t(cap * 11), d_decode=t(cap * 16),
                     d_work=t(cap * 100 * 8))
        else:
            a = dict(d_hits=t(cap * 16), d_rows=t(cap * 11), d_results=t(560), n_groups=1, max_frames=cap,
                     sync_len=8, frame_symbols=N, len_bytes=1, crc=A.DEMOD_CRC16_CCITT_FALSE,
                     d_check=t(cap * 16), d_kept=t(cap, torch.int32), d_body=None, d_summary=t(32))
        a.update(kw)
        with pytest.raises(A.DemodError) as e:
            getattr(d, fn)(**a)
        assert e.value.code == A.DEMOD_BAD_ARG
        return str(e.value)

    for fn in ("frames_decode_async", "frames_check_coded_async"):
        assert "d_hits" in call(fn)                       # host tensors: the first one is refused
        for kw in (dict(n_groups=0), dict(n_groups=A.DEMOD_MAX_SEGMENTS + 1), dict(max_frames=0),
                   dict(n_groups=2 ** 15, max_frames=2 ** 16), dict(frame_symbols=-1)):
            assert "n_groups" in call(fn, **kw)
        for kw in (dict(len_bytes=0), dict(len_bytes=3), dict(crc=0), dict(crc=7)):
            assert "len_bytes" in call(fn, **kw)
        assert "look-ahead" in call(fn, frame_symbols=143)
        assert "look-ahead" in call(fn, frame_symbols=159, len_bytes=2)
        assert "max_len" in call(fn, frame_symbols=2 * (8 * 4100 + 6))
        assert "fec" in call(fn, fec=0) and "fec" in call(fn, fec=2)
        assert "raw address" in call(fn, d_hits=1234)
        assert "required" in call(fn, d_hits=None)
    assert "n_windows" in call(n_windows=2 ** 31) and "n_windows" in call(n_windows=-1)
    five = object.__new__(A.Demodulator)
    five._lib, five._h = d._lib, None
    five.cfg = A.make_cfg(n=1024, hop=256, freqs=tuple(1500.0 + 375.0 * i for i in range(5)))
    with pytest.raises(A.DemodError) as e:
        five.frames_coded(np.zeros(8192, np.int16), [0, 1], frame_symbols=400)
    assert "2^bits" in str(e.value)
    for kw in (dict(frame_symbols=143), dict(frame_symbols=400, max_frames=0), dict(frame_symbols=400, fec=0)):
        with pytest.raises(A.DemodError):
            d.frames_coded(np.zeros(8192, np.int16), [0, 1], **kw)


def test_standalone_program_under_sanitizers(tmp_path):
    """tests/native/fec_host_test.c with the host sources, built with
    -fsanitize=address,undefined and run as a program of its own."""
    csrc = os.path.join(ROOT, "audio-network_amd", "csrc")
    exe = str(tmp_path / "fec_host_test")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "native", "fec_host_test.c"), os.path.join(csrc, "demod_fec.c"),
                    os.path.join(csrc, "demod_frame_check.c"), os.path.join(csrc, "demod_frame.c"),
                    "-lm", "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "300", "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "fec_host_test OK" in r.stdout
