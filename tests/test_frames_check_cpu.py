"""Checked frames without a GPU: the ABI (exports, struct layouts), demod_crc
and demod_checked_frame_encode against tests/frames_check_ref.py's bitwise
restatement, the round trip through the symbol packing, the reference's
covered rule on hand-made cases, and what the Python mirror of
demod_frames_check_async refuses before any pointer reaches the library."""
import binascii
import ctypes

import numpy as np
import pytest

import fec_modes_ref as Z
import frames_check_ref as C

KINDS = (C.CRC16, C.CRC32)


def test_exports_and_structs(A):
    lib = A.load_library()
    for name in ("demod_crc", "demod_checked_frame_size", "demod_checked_frame_encode",
                 "demod_frames_check_async", "demod_frames_checked"):
        assert hasattr(lib, name), name
        assert name in A.header_exports()
    for name in ("frames_check_async", "frames_checked"):
        assert callable(getattr(A.Demodulator, name))
    T, S = A.DemodFrameCheck, A.DemodFramesCheckResult
    assert ctypes.sizeof(T) == 16 and ctypes.sizeof(S) == 32
    assert (T.length.offset, T.crc.offset, T.status.offset, T.covered.offset) == (0, 4, 8, 12)
    assert (S.n_checked.offset, S.n_valid.offset, S.n_kept.offset, S.reserved.offset) == (0, 8, 16, 24)
    assert A.FRAME_CHECK_DTYPE == C.CHECK_DTYPE and A.FRAMES_CHECK_RESULT_DTYPE == C.SUMMARY_DTYPE
    assert (A.DEMOD_CRC16_CCITT_FALSE, A.DEMOD_CRC32_MPEG2) == (C.CRC16, C.CRC32) == (1, 2)
    assert (A.DEMOD_CHECK_OK, A.DEMOD_CHECK_BAD_LENGTH, A.DEMOD_CHECK_BAD_CRC) == (C.OK, C.BAD_LENGTH,
                                                                                   C.BAD_CRC) == (0, 1, 2)
    assert A.CRC_BYTES == C.CRC_BYTES
    assert lib.demod_frames_check_async(None, None, None, None, 1, 1, 1, 64, 1, 1, None, None, None, None,
                                        None) == A.DEMOD_BAD_ARG
    res, summ = A.DemodFramesResult(), A.DemodFramesCheckResult()
    assert lib.demod_frames_checked(None, None, 4, None, 0, 0, 64, 1, 1, None, None, None, 1,
                                    ctypes.byref(res), ctypes.byref(summ)) == A.DEMOD_BAD_ARG


def test_crc_check_values(A):
    assert C.crc(C.CRC16, b"123456789") == 0x29B1 == A.crc(A.DEMOD_CRC16_CCITT_FALSE, b"123456789")
    assert C.crc(C.CRC32, b"123456789") == 0x0376E6E7 == A.crc(A.DEMOD_CRC32_MPEG2, b"123456789")
    assert A.crc(C.CRC16, b"") == C.crc(C.CRC16, b"") == 0xFFFF
    assert A.crc(C.CRC32, b"") == C.crc(C.CRC32, b"") == 0xFFFFFFFF
    assert A.load_library().demod_crc(0, None, 0) == 0 and A.load_library().demod_crc(3, None, 0) == 0
    with pytest.raises(A.DemodError):
        A.crc(0, b"x")


def test_crc_random_lengths(A):
    rng = np.random.default_rng(11)
    lengths = [1, 2, 3, 63, 64, 65, 130, 1000, 4102, 4200] + rng.integers(1, 4201, 30).tolist()
    for n in lengths:
        d = rng.integers(0, 256, n).astype(np.uint8).tobytes()
        for kind in KINDS:
            assert A.crc(kind, d) == C.crc(kind, d), (kind, n)
        assert A.crc(C.CRC16, d) == binascii.crc_hqx(d, 0xFFFF)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h", [1, 2])
def test_encode(A, h, kind):
    rng = np.random.default_rng(100 * h + kind)
    c = C.CRC_BYTES[kind]
    for n in (0, 1, 255, 256, 4096, 4097):
        d = rng.integers(0, 256, n).astype(np.uint8).tobytes()
        want = C.encode(d, h, kind)
        if (h == 1 and n >= 256) or n == 4097:
            assert want is None
            with pytest.raises(A.DemodError) as e:
                A.checked_frame_encode(d, h, kind)
            assert e.value.code == A.DEMOD_FRAME_TOO_LARGE
            with pytest.raises(A.DemodError):
                A.checked_frame_size(n, h, kind)
            continue
        got = A.checked_frame_encode(d, h, kind)
        assert got == want and len(got) == h + n + c == A.checked_frame_size(n, h, kind)
        assert int.from_bytes(got[:h], "big") == n and got[h:h + n] == d
        assert C.check_row(got, h, kind) == (n, C.crc(kind, got[:h + n]), C.OK)
        # the room it needs exactly, and one byte less
        assert A.checked_frame_encode(d, h, kind, cap=len(want)) == want
        with pytest.raises(A.DemodError) as e:
            A.checked_frame_encode(d, h, kind, cap=len(want) - 1)
        assert e.value.code == A.DEMOD_BUFFER_TOO_SMALL
    for bad in (dict(len_bytes=0), dict(len_bytes=3), dict(crc=0), dict(crc=3)):
        kw = dict(len_bytes=h, crc=kind)
        kw.update(bad)
        with pytest.raises(A.DemodError) as e:
            A.checked_frame_encode(b"abc", **kw)
        assert e.value.code == A.DEMOD_BAD_ARG
        with pytest.raises(A.DemodError):
            A.checked_frame_size(3, **kw)
    lib = A.load_library()
    out = (ctypes.c_uint8 * 16)()
    assert lib.demod_checked_frame_encode(None, 3, h, kind, out, 16) == A.DEMOD_BAD_ARG
    assert lib.demod_checked_frame_encode(None, 0, h, kind, None, 16) == A.DEMOD_BAD_ARG
    assert lib.demod_checked_frame_encode(None, 0, h, kind, out, 16) == h + c


@pytest.mark.parametrize("bits", [1, 3, 4])
def test_round_trip_through_symbols(A, bits):
    """encode -> unpack_symbols -> (a row padded with random symbols) ->
    pack_symbols is a row the reference accepts, with the data in place."""
    rng = np.random.default_rng(bits)
    for kind in KINDS:
        for h in (1, 2):
            for n in (0, 1, 7, 100, 255):
                d = rng.integers(0, 256, n).astype(np.uint8).tobytes()
                frame = A.checked_frame_encode(d, h, kind)
                S = C.frame_symbols(len(frame), bits)
                # (the last symbol's missing bits are 0: one more byte for the library's reader)
                sym = A.unpack_symbols(frame + bytes(1), S, bits)
                assert np.array_equal(sym, C.unpack(frame, S, bits))
                N = S + int(rng.integers(0, 9))
                row = C.payload_row(frame, N, bits, rng)
                assert np.array_equal(row[:S], sym)
                packed = A.pack_symbols(row, bits)
                assert packed == C.pack(row, bits)
                length, got, status = C.check_row(packed, h, kind)
                assert (length, status) == (n, C.OK) and got == A.crc(kind, frame[:h + n])
                assert packed[h:h + n] == d


def rows_of(frames, B):
    return np.array([list(f + bytes(B - len(f))) for f in frames], np.uint8)


def test_covered_rule():
    """L = 4, R = 4, bits = 1, h = 1, CRC-16: a frame of len data bytes
    occupies 4 + (3 + len) 8 symbols, (28 + 8 len) 4 windows."""
    L, R, bits, h, kind, B = 4, 4, 1, 1, C.CRC16, 12
    plain = Z.span_of(bits, h, kind, 0)
    good = [C.encode(bytes([i] * n), h, kind) for i, n in enumerate((2, 0, 5, 1))]
    span = [(L + C.frame_symbols(len(f), bits)) * R for f in good]
    assert span == [(28 + 8 * n) * 4 for n in (2, 0, 5, 1)]
    bad = bytearray(good[2])
    bad[3] ^= 0x10
    # touching frames: the second starts at the first's end
    chk, kept, bodies, summ = C.check_group([10, 10 + span[0]], rows_of(good[:2], B), L, R, plain, None, h, kind)
    assert chk["covered"].tolist() == [0, 0] and kept.tolist() == [0, 1]
    assert bodies == [bytes([0, 0]), b""]
    assert summ.tolist() == (2, 2, 2, 0)
    # one window of overlap
    chk, kept, _, summ = C.check_group([10, 10 + span[0] - 1], rows_of(good[:2], B), L, R, plain, None, h, kind)
    assert chk["covered"].tolist() == [0, 1] and kept.tolist() == [0] and summ.tolist() == (2, 2, 1, 0)
    # an invalid frame in between covers nothing, and is not covered
    w = [10, 10 + span[0], 10 + span[0] + 4]
    chk, kept, _, summ = C.check_group(w, rows_of([good[0], bytes(bad), good[3]], B), L, R, plain, None, h, kind)
    assert chk["status"].tolist() == [C.OK, C.BAD_CRC, C.OK]
    assert chk["covered"].tolist() == [0, 0, 0] and kept.tolist() == [0, 2] and summ.tolist() == (3, 2, 2, 0)
    # the same place with a valid frame there: the third is covered
    chk, kept, _, _ = C.check_group(w, rows_of([good[0], good[2], good[3]], B), L, R, plain, None, h, kind)
    assert chk["covered"].tolist() == [0, 0, 1] and kept.tolist() == [0, 1]
    # a covered frame still covers (prefix maximum, not the greedy hold-off): row 1 is
    # inside row 0, row 2 is past row 0's end but inside row 1
    w = [0, span[0] - 4, span[0] + 4]
    chk, kept, _, _ = C.check_group(w, rows_of([good[0], good[2], good[3]], B), L, R, plain, None, h, kind)
    assert chk["covered"].tolist() == [0, 1, 1] and kept.tolist() == [0]
    # a bad length reads nothing past the header
    long_row = bytes([B - h - 2 + 1]) + bytes(B - 1)
    chk, kept, _, summ = C.check_group([0], rows_of([long_row], B), L, R, plain, None, h, kind)
    assert chk[0].tolist() == (B - 2, 0, C.BAD_LENGTH, 0) and kept.size == 0 and summ.tolist() == (1, 0, 0, 0)
    # ends wrap at 2^64 as the device's do
    chk, _, _, _ = C.check_group([2 ** 64 - 8, 2 ** 64 - 4], rows_of(good[:2], B), L, R, plain, None, h, kind)
    assert chk["covered"].tolist() == [0, 0]


def test_python_mirror_refuses_before_the_library(A):
    """No device here: every path of Demodulator.frames_check_async ends in the
    mirror's own checks (the C refusals are tests/test_gpu_frames_check.py's)."""
    torch = pytest.importorskip("torch")
    d = object.__new__(A.Demodulator)
    d._lib, d.cfg, d._h = A.load_library(), A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS), None
    N, cap = 64, 4

    def t(nbytes, dtype=torch.uint8):
        return torch.zeros(nbytes, dtype=dtype)

    def call(**kw):
        a = dict(d_hits=t(cap * 16), d_packed=t(cap * 8), d_results=t(560), n_groups=1, max_frames=cap,
                 sync_len=8, frame_symbols=N, len_bytes=1, crc=A.DEMOD_CRC16_CCITT_FALSE,
                 d_check=t(cap * 16), d_kept=t(cap, torch.int32), d_body=None, d_summary=t(32))
        a.update(kw)
        with pytest.raises(A.DemodError) as e:
            d.frames_check_async(**a)
        assert e.value.code == A.DEMOD_BAD_ARG
        return str(e.value)

    assert "d_hits" in call()                             # host tensors: the first one is refused
    for kw in (dict(n_groups=0), dict(n_groups=A.DEMOD_MAX_SEGMENTS + 1), dict(max_frames=0),
               dict(n_groups=2 ** 15, max_frames=2 ** 16), dict(frame_symbols=-1)):
        assert "n_groups" in call(**kw)
    for kw in (dict(len_bytes=0), dict(len_bytes=3), dict(crc=0), dict(crc=7)):
        assert "len_bytes" in call(**kw)
    for kw in (dict(frame_symbols=16), dict(frame_symbols=8 * 4100), dict(frame_symbols=40, len_bytes=2, crc=2)):
        assert "rows too short" in call(**kw)
    assert "raw address" in call(d_hits=1234)
    assert "required" in call(d_hits=None)
    with pytest.raises(A.DemodError):
        d.frames_checked(np.zeros(4096, np.int16), [0, 1], frame_symbols=16)
    with pytest.raises(A.DemodError):
        d.frames_checked(np.zeros(4096, np.int16), [0, 1], frame_symbols=64, max_frames=0)
