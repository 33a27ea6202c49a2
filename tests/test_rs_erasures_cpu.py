"""Erasure decoding on the host (include/demod.h "erasure decoding"):
demod_rs_frame_decode_erasures against the independent reference
tests/rs_erasure_ref.py (another algorithm) and its decoder-free checker, bit
for bit in the rows and in both records; a NULL and an all-zero mask against
demod_rs_frame_decode; demod_soft_erasures against a numpy restatement; the
gain through the host chain alone; the refusals; the host sources in a
stand-alone program under AddressSanitizer and UBSan
(tests/native/rs_erasure_host_test.c); and a seeded study of the level, which
is reported and not asserted.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import frames_check_ref as C
import rs_cases as RC
import rs_erasure_cases as EC
import rs_erasure_ref as E
import rs_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS, FLAGS = RC.KINDS, RC.FLAGS


def test_exports_and_constants(A):
    lib = A.load_library()
    for name in ("demod_rs_frame_decode_erasures", "demod_soft_erasures", "demod_frames_erasures_async",
                 "demod_frames_rs_erasures_async"):
        assert hasattr(lib, name), name
        assert name in A.header_exports()
    assert A.DEMOD_FEC_ERASE(1) == 1 << 16 and A.DEMOD_FEC_ERASE(127) == 127 << 16 and A.DEMOD_FEC_ERASE(128) == 0
    assert ctypes.sizeof(A.DemodFrameErase) == 16
    assert A.FRAME_ERASE_DTYPE.names == ("erased", "used", "fallback", "reserved")
    assert [A.mask_words(b) for b in (1, 64, 65, 4710)] == [1, 1, 2, 74]
    flags = np.zeros(130, bool)
    flags[[0, 63, 64, 129]] = True
    assert A.pack_mask(flags, 130).tolist() == E.pack_mask(flags.tolist(), 130) == [1 | 1 << 63, 1, 2]


# ---- the decoder against the reference ---------------------------------------------------

def frames_of(P):
    """(h, kind, len): the shortest frame (one codeword of k = h + c = 3 message bytes, the fewest a frame
    can have: k_j = 1 needs n < 2 D, which no frame of n >= 3 bytes has), D = 1 full, D = 2 and D = 5 with
    unequal k_j."""
    kmax = 255 - P
    five = 4 * kmax + 17
    five += (2 + five + 4) % 5 == 0
    return [(1, C.CRC16, 0), (1, C.CRC32, kmax - 5), (2, C.CRC16, kmax + 2), (2, C.CRC32, five)]


def decode_and_compare(A, row, flags, h, kind, flag):
    P = R.PARITY[flag]
    got, rec, erec, covered = A.rs_frame_decode(bytes(row), h, kind, flag, erase=np.asarray(flags, bool))
    want, wrec, werec = E.frame_decode(bytes(row), h, kind, P, list(flags))
    assert bytes(got) == want, "the rows differ"
    assert rec == wrec and erec == werec, (rec, wrec, erec, werec)
    E.check_frame(bytes(row), bytes(got), list(flags), rec, erec, h, kind, P)
    return bytes(got), rec, erec, covered


@pytest.mark.parametrize("flag", FLAGS)
def test_decoder_equals_the_reference(A, flag):
    """Rows and both records, bit for bit, over f in {0, 1, P - 1, P, P + 1} and
    2 e + f at, one error past and two errors past the limit in every codeword;
    flags on right bytes, on parity, on header bytes and past n'. Beyond the
    limit the expected outcome is whatever the reference says."""
    P = R.PARITY[flag]
    rng = np.random.default_rng(300 + P)
    seen = set()
    for h, kind, length in frames_of(P):
        c = C.CRC_BYTES[kind]
        n = h + length + c
        D = R.codewords(n, P)
        if D > 1:
            assert n % D != 0, "unequal k_j"
        data = bytes(rng.integers(0, 256, length, dtype=np.uint8))
        sent = A.rs_frame_encode(data, h, kind, flag)
        assert len(sent) == R.frame_size(n, P)
        for plan in EC.rounds(P, D):
            row = bytearray(sent + bytes(rng.integers(0, 256, 7, dtype=np.uint8)))
            flags = np.zeros(len(row), bool)
            flags[len(sent):] = rng.integers(0, 2, 7).astype(bool)          # past n': ignored
            planted = EC.plant(row, flags, n, P, h, rng, plan)
            got, rec, erec, covered = decode_and_compare(A, row, flags, h, kind, flag)
            assert covered == len(sent) and erec["erased"] == sum(f for f, _ in planted)
            if all(2 * e + f <= P for f, e in planted):
                assert got[:len(sent)] == sent
            seen |= {(f, min(2 * e + f, P + 3)) for f, e in planted}
        # the header bytes flagged and right, and every parity byte of codeword 0 flagged
        row = bytearray(sent)
        flags = np.zeros(len(row), bool)
        flags[:h] = True
        flags[[n + i * D for i in range(P - h)]] = True
        row[n] ^= 0x5A
        got, rec, erec, _ = decode_and_compare(A, row, flags, h, kind, flag)
        assert got == sent and erec["used"] == 1 and rec["corrected"] == 1
    for f in (0, 1, P - 1, P, P + 1):
        assert any(g == f for g, _ in seen), f
    assert {(1, P - 1), (1, P + 1), (P, P), (P, P + 2), (0, P), (0, P + 2)} <= seen


def test_decoder_at_the_payload_limit(A):
    """n' = 4710: P = 32, D = 19, h = 2, CRC-32, once."""
    flag, P, h, kind = R.FLAG32, 32, 2, C.CRC32
    rng = np.random.default_rng(19)
    sent = A.rs_frame_encode(bytes(rng.integers(0, 256, 4096, dtype=np.uint8)), h, kind, flag)
    assert len(sent) == 4710 and R.codewords(4102, P) == 19
    row, flags = bytearray(sent), np.zeros(4710, bool)
    EC.plant(row, flags, 4102, P, h, rng, EC.combos(P))
    decode_and_compare(A, row, flags, h, kind, flag)


def test_random_masks_and_errors(A):
    """Seeded random masks and errors of any weight, every mode with a parity flag."""
    rng = np.random.default_rng(77)
    for trial in range(24):
        fec = A.RS_PARITY_MODES[trial % len(A.RS_PARITY_MODES)]
        flag = fec & 0x300
        P, h, kind = R.PARITY[flag], 1 + trial % 2, KINDS[trial % 2]
        length = int(rng.integers(0, 300 if h == 2 else 200))
        sent = A.rs_frame_encode(bytes(rng.integers(0, 256, length, dtype=np.uint8)), h, kind, flag)
        row = bytearray(sent + bytes(3))
        flags = rng.random(len(row)) < rng.choice([0.01, 0.05, 0.12])
        for b in np.flatnonzero(rng.random(len(sent)) < rng.choice([0.01, 0.04, 0.08])):
            if b >= h:
                row[b] ^= int(rng.integers(1, 256))
        P_ = R.PARITY[flag]
        got, rec, erec, _ = A.rs_frame_decode(bytes(row), h, kind, fec, erase=flags)
        want, wrec, werec = E.frame_decode(bytes(row), h, kind, P_, flags.tolist())
        assert (bytes(got), rec, erec) == (want, wrec, werec), trial
        E.check_frame(bytes(row), bytes(got), flags.tolist(), rec, erec, h, kind, P_)


# ---- compatibility ---------------------------------------------------------------------------

@pytest.mark.parametrize("flag", FLAGS)
def test_null_and_zero_masks_are_the_plain_decoder(A, flag):
    lib = A.load_library()
    P = R.PARITY[flag]
    rng = np.random.default_rng(5 + P)
    for h in (1, 2):
        for kind in KINDS:
            c = C.CRC_BYTES[kind]
            for length in RC.edge_lengths(h, c, P)[:5]:
                sent = A.rs_frame_encode(bytes(rng.integers(0, 256, length, dtype=np.uint8)), h, kind, flag)
                for pattern in RC.PATTERNS:
                    row = bytearray(sent + bytes(5))
                    RC.corrupt(row, h + length + c, P, h, pattern, rng)
                    want, wrec, wn = A.rs_frame_decode(bytes(row), h, kind, flag)
                    zero = np.zeros(A.mask_words(len(row)), np.uint64)
                    for erase in (None, zero.ctypes.data):
                        buf = np.frombuffer(bytes(row), np.uint8).copy()
                        rec, erec = A.DemodFrameRs(), A.DemodFrameErase(9, 9, 9, 9)
                        n = lib.demod_rs_frame_decode_erasures(buf.ctypes.data, buf.size, h, kind, flag, erase,
                                                               ctypes.byref(rec), ctypes.byref(erec))
                        assert n == wn and np.array_equal(buf, want) and A._struct_dict(rec) == wrec
                        assert A._struct_dict(erec) == dict(erased=0, used=0, fallback=0, reserved=0)


# ---- the mask from soft values -------------------------------------------------------------------

@pytest.mark.parametrize("k", (2, 4, 8, 16))
def test_soft_erasures_against_numpy(A, k):
    bits = {2: 1, 4: 2, 8: 3, 16: 4}[k]
    rng = np.random.default_rng(k)
    N = {1: 1035, 2: 531, 3: 347, 4: 261}[bits]          # N bits is not a multiple of 8; more than 64 bytes
    assert (N * bits) % 8 != 0
    powers = rng.random((N, k), dtype=np.float32) ** 4
    powers[5] = 0.0                                      # q = 0
    powers[6] = 3.0
    soft = np.concatenate([A.soft_bits(powers[j]) for j in range(N)])
    assert soft.size == N * bits
    B = (N * bits + 7) // 8
    for level in (1, 64, 127):
        for row_bytes in (B, B + 70, B - 1):
            padded = np.zeros(8 * max(row_bytes, B), np.int64)
            padded[:soft.size] = np.abs(soft.astype(np.int64))
            want = padded[:8 * row_bytes].reshape(row_bytes, 8).min(axis=1) < level
            got = A.soft_erasures(soft, level, row_bytes)
            assert got.tolist() == E.pack_mask(want.tolist(), row_bytes), (level, row_bytes)
            if row_bytes >= B:
                assert want[B - 1] and want[B:].all()    # the padded byte and the bytes past the row's soft values


# ---- the gain, through the host chain alone ------------------------------------------------------

def crc_ok(A, row, h, kind):
    c = C.CRC_BYTES[kind]
    length = int.from_bytes(row[:h], "big")
    if h + length + c > len(row):
        return False
    return A.crc(kind, bytes(row[:h + length])) == int.from_bytes(row[h + length:h + length + c], "big")


def test_gain_nine_to_sixteen_lost_bytes(A):
    """DEMOD_FEC_RS16: 9 to 16 wrong bytes in the one codeword come back when
    they are flagged and lose the frame when they are not."""
    rng = np.random.default_rng(16)
    data = bytes(rng.integers(0, 256, 120, dtype=np.uint8))
    sent = A.rs_frame_encode(data, 1, C.CRC16, 0x100)
    for wrong in range(9, 17):
        where = rng.choice(np.arange(1, len(sent)), wrong, replace=False)
        row = bytearray(sent)
        for b in where:
            row[b] ^= int(rng.integers(1, 256))
        flags = np.zeros(len(row), bool)
        flags[where] = True
        got, rec, erec, _ = A.rs_frame_decode(bytes(row), 1, C.CRC16, 0x100, erase=flags)
        assert bytes(got) == sent and crc_ok(A, bytes(got), 1, C.CRC16)
        assert rec == dict(status=R.OK, codewords=1, corrected=wrong, failed=0)
        assert erec == dict(erased=wrong, used=1, fallback=0, reserved=0)
        got, rec, _ = A.rs_frame_decode(bytes(row), 1, C.CRC16, 0x100)
        assert rec["status"] == R.FAILED and bytes(got) == bytes(row) and not crc_ok(A, bytes(got), 1, C.CRC16)


def test_gain_a_run_of_d_times_p_bytes(A):
    """D = 3 at P = 16: a run of D P = 48 consecutive lost bytes, flagged, comes
    back over the byte interleave; unflagged, the frame is lost."""
    rng = np.random.default_rng(48)
    data = bytes(rng.integers(0, 256, 600, dtype=np.uint8))
    sent = A.rs_frame_encode(data, 2, C.CRC16, 0x100)
    assert R.codewords(604, 16) == 3
    row = bytearray(sent)
    for b in range(100, 148):
        row[b] ^= int(rng.integers(1, 256))
    flags = np.zeros(len(row), bool)
    flags[100:148] = True
    got, rec, erec, _ = A.rs_frame_decode(bytes(row), 2, C.CRC16, 0x100, erase=flags)
    assert bytes(got) == sent and rec == dict(status=R.OK, codewords=3, corrected=48, failed=0)
    assert erec == dict(erased=48, used=3, fallback=0, reserved=0)
    got, rec, _ = A.rs_frame_decode(bytes(row), 2, C.CRC16, 0x100)
    assert rec == dict(status=R.FAILED, codewords=3, corrected=0, failed=3) and not crc_ok(A, bytes(got), 2, C.CRC16)


# ---- refusals ------------------------------------------------------------------------------------

def test_refusals(A):
    lib = A.load_library()
    cfg2 = A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS)
    word = [0, 1, 1, 0, 1]
    rx_base = dict(sync=word, max_errors=0, frame_symbols=1024, len_bytes=1, crc=C.CRC16, max_frames=4,
                   ring_windows=2 * 1029 * 4)
    tx_base = dict(sync=word, len_bytes=1, crc=C.CRC16, max_len=16, ring_symbols=8192)
    lv = A.DEMOD_FEC_ERASE(16)
    d = object.__new__(A.Demodulator)
    d._lib, d.cfg, d._h = lib, cfg2, None
    # the receiver's size function and the one-shot call's mirror take a level with a parity flag alone
    for fec in (0x100 | lv, 0x200 | A.DEMOD_FEC_ERASE(127), 0x100 | A.DEMOD_FEC_ERASE(1)):
        z = A.rx_sizes(cfg2, A.make_rx_cfg(fec=fec, **rx_base), 2)
        assert z == A.rx_sizes(cfg2, A.make_rx_cfg(fec=fec & 0xFFFF, **rx_base), 2)
        assert A.erase_mode_parts(fec) == (fec & 0xFFFF, fec >> 16)
    # a level without a parity flag, with the convolutional code, and beside an unknown bit
    for fec in (lv, lv | 1, lv | 0x101, lv | 0x241, lv | 0x300, lv | 0x100 | 1 << 23, lv | 0x100 | 0x400):
        with pytest.raises(A.DemodError):
            A.rx_sizes(cfg2, A.make_rx_cfg(fec=fec, **rx_base), 2)
        with pytest.raises(A.DemodError):
            A.erase_mode_parts(fec)
        with pytest.raises(A.DemodError) as e:
            d.frames_coded(np.zeros(8192, np.int16), word, frame_symbols=1024, fec=fec)
        assert "fec" in str(e.value)
    # every other entry refuses the field as it refuses any unknown bit
    fec = 0x100 | lv
    out = (ctypes.c_uint8 * 64)()
    rec, erec = A.DemodFrameRs(), A.DemodFrameErase()
    words = np.zeros(1, np.uint64)
    assert lib.demod_rs_frame_size(0, 1, C.CRC16, fec) == A.DEMOD_BAD_ARG
    assert lib.demod_rs_max_len(64, 1, C.CRC16, fec) == A.DEMOD_BAD_ARG
    assert lib.demod_rs_frame_encode(None, 0, 1, C.CRC16, fec, out, 64) == A.DEMOD_BAD_ARG
    assert lib.demod_rs_frame_decode(out, 64, 1, C.CRC16, fec, ctypes.byref(rec)) == A.DEMOD_BAD_ARG
    assert lib.demod_rs_frame_decode_erasures(out, 64, 1, C.CRC16, fec, words.ctypes.data, ctypes.byref(rec),
                                              ctypes.byref(erec)) == A.DEMOD_BAD_ARG
    assert lib.demod_fec_frame_symbols(0, 1, C.CRC16, 1, fec | 1) == A.DEMOD_BAD_ARG
    assert lib.demod_fec_row_bytes(1024, 1, 1, fec | 1) == A.DEMOD_BAD_ARG
    assert lib.demod_fec_decode_workspace_size(ctypes.byref(cfg2), 1, 4, 1024, fec | 1) == 0
    with pytest.raises(A.DemodError):
        A.tx_sizes(cfg2, A.make_tx_cfg(fec=fec, **tx_base), 2)
    with pytest.raises(A.DemodError):
        A.tx_frame_symbols(A.make_tx_cfg(fec=fec, **tx_base), 2, b"ab")
    for call in (lambda: d.frames_rs_async(None, None, 1, 4, 1024, 1, C.CRC16, fec, None),
                 lambda: d.frames_rs_erasures_async(None, None, None, 1, 4, 1024, 1, C.CRC16, fec, None, None),
                 lambda: d.frames_check_coded_async(None, None, None, 1, 4, 5, 1024, 1, C.CRC16, None, None, None,
                                                    None, fec=fec),
                 lambda: d.rx_collect_async(None, None, None, None, None, None, None, 1, 4, 5, 1024, 1, C.CRC16,
                                            fec, None, None, None, None)):
        with pytest.raises(A.DemodError) as e:
            call()
        assert "fec" in str(e.value)
    # the erasure decoder: a mode without a parity flag, NULL and misaligned pointers
    row = np.zeros(64, np.uint8)
    two = np.zeros(2, np.uint64)
    ok = (row.ctypes.data, 64, 1, C.CRC16, 0x100)
    assert lib.demod_rs_frame_decode_erasures(*ok, two.ctypes.data, ctypes.byref(rec), ctypes.byref(erec)) > 0
    assert lib.demod_rs_frame_decode_erasures(row.ctypes.data, 64, 1, C.CRC16, 1, two.ctypes.data,
                                              ctypes.byref(rec), ctypes.byref(erec)) == A.DEMOD_BAD_ARG
    assert lib.demod_rs_frame_decode_erasures(*ok, two.ctypes.data + 4, ctypes.byref(rec),
                                              ctypes.byref(erec)) == A.DEMOD_BAD_ARG
    assert lib.demod_rs_frame_decode_erasures(*ok, two.ctypes.data, None, ctypes.byref(erec)) == A.DEMOD_BAD_ARG
    assert lib.demod_rs_frame_decode_erasures(*ok, two.ctypes.data, ctypes.byref(rec), None) == A.DEMOD_BAD_ARG
    assert lib.demod_rs_frame_decode_erasures(None, 64, 1, C.CRC16, 0x100, two.ctypes.data, ctypes.byref(rec),
                                              ctypes.byref(erec)) == A.DEMOD_BAD_ARG
    # demod_soft_erasures: level 0 and 128, NULL and misaligned pointers, no row
    soft = np.zeros(64, np.int8)
    assert lib.demod_soft_erasures(soft.ctypes.data, 64, 1, two.ctypes.data, 8) == 1
    for level in (0, -1, 128):
        assert lib.demod_soft_erasures(soft.ctypes.data, 64, level, two.ctypes.data, 8) == A.DEMOD_BAD_ARG
        with pytest.raises(A.DemodError):
            A.soft_erasures(soft, level, 8)
    assert lib.demod_soft_erasures(None, 64, 1, two.ctypes.data, 8) == A.DEMOD_BAD_ARG
    assert lib.demod_soft_erasures(soft.ctypes.data, 64, 1, None, 8) == A.DEMOD_BAD_ARG
    assert lib.demod_soft_erasures(soft.ctypes.data, 64, 1, two.ctypes.data + 4, 8) == A.DEMOD_BAD_ARG
    assert lib.demod_soft_erasures(soft.ctypes.data, 64, 1, two.ctypes.data, 0) == A.DEMOD_BAD_ARG
    # the producer's mirror judges the level before any tensor
    for level in (0, 128):
        with pytest.raises(A.DemodError) as e:
            d.frames_erasures_async(None, None, 16, None, None, 1, 4, 5, 1024, level, None)
        assert "level" in str(e.value)


def test_level_at_the_widest_rows(A):
    """The level is taken at every row width its mode takes, up to n' = 4710 at
    DEMOD_FEC_RS32 (a fec-0 row stops at 4102 bytes), and the sizes are the
    mode's without the field; one symbol more is refused as it is without it.
    K = 3 has no soft values: the level is refused there, the mode is not."""
    cfg2 = A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS)
    word = [0, 1, 1, 0, 1]
    for fec, h, kind, B in ((0x200, 2, C.CRC32, 4710), (0x200, 2, C.CRC16, 4708), (0x100, 2, C.CRC32, 4390),
                            (0x100, 1, C.CRC16, 4200)):
        base = dict(sync=word, max_errors=0, len_bytes=h, crc=kind, max_frames=2,
                    ring_windows=2 * (5 + 8 * B + 8) * 4)
        plain = A.rx_sizes(cfg2, A.make_rx_cfg(fec=fec, frame_symbols=8 * B, **base), 1)
        assert plain["row_bytes"] == B
        assert A.rx_sizes(cfg2, A.make_rx_cfg(fec=fec | A.DEMOD_FEC_ERASE(16), frame_symbols=8 * B, **base), 1) == plain
        if h == 2:
            for mode in (fec, fec | A.DEMOD_FEC_ERASE(16)):
                with pytest.raises(A.DemodError):
                    A.rx_sizes(cfg2, A.make_rx_cfg(fec=mode, frame_symbols=8 * (B + 1), **base), 1)
    d = object.__new__(A.Demodulator)
    d._lib, d.cfg, d._h = A.load_library(), cfg2, None
    with pytest.raises(A.DemodError) as e:       # the mirror takes the widest row: it fails on the tensors, not on N
        d.frames_erasures_async(None, None, 16, None, None, 1, 4, 5, 8 * 4710, 16, None)
    assert "frame_symbols" not in str(e.value)
    with pytest.raises(A.DemodError) as e:
        d.frames_erasures_async(None, None, 16, None, None, 1, 4, 5, 8 * 4710 + 1, 16, None)
    assert "frame_symbols" in str(e.value)
    cfg3 = A.make_cfg(n=1024, hop=256, freqs=(1500.0, 1875.0, 2250.0))
    base = dict(sync=word, max_errors=0, len_bytes=1, crc=C.CRC16, max_frames=2, frame_symbols=1024,
                ring_windows=2 * 1029 * 4)
    A.rx_sizes(cfg3, A.make_rx_cfg(fec=0x100, **base), 1)
    with pytest.raises(A.DemodError):
        A.rx_sizes(cfg3, A.make_rx_cfg(fec=0x100 | A.DEMOD_FEC_ERASE(16), **base), 1)


# ---- the host sources under sanitizers -----------------------------------------------------------

def test_standalone_program_under_sanitizers(tmp_path):
    """tests/native/rs_erasure_host_test.c with the host sources, built with
    -fsanitize=address,undefined and run as a program of its own."""
    csrc = os.path.join(ROOT, "audio-network_amd", "csrc")
    exe = str(tmp_path / "rs_erasure_host_test")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "native", "rs_erasure_host_test.c"), os.path.join(csrc, "demod_rs.c"),
                    os.path.join(csrc, "demod_fec.c"), os.path.join(csrc, "demod_tx_frame.c"),
                    os.path.join(csrc, "demod_frame_check.c"), os.path.join(csrc, "demod_frame.c"), "-lm",
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "rs_erasure_host_test OK" in r.stdout


# ---- a study of the level: reported, not asserted ------------------------------------------------

def level_study(A, trials=40, seed=2026):
    """24-byte blocks at DEMOD_FEC_RS16 over 2-FSK tone powers with noise: a
    fade of `length` symbols that scales the signal's power by `depth`, the
    frames lost with errors only and at levels 16, 32 and 64. Returns rows of
    (length, depth, lost at errors-only, at 16, at 32, at 64) out of `trials`."""
    rng = np.random.default_rng(seed)
    table = []
    for length in (32, 64, 96, 128, 160):
        for depth in (0.25, 0.05, 0.0):
            lost = [0, 0, 0, 0]
            for _ in range(trials):
                data = bytes(rng.integers(0, 256, 24, dtype=np.uint8))
                sent = A.rs_frame_encode(data, 1, C.CRC16, 0x100)
                bits = np.unpackbits(np.frombuffer(sent, np.uint8))
                gain = np.ones(bits.size)
                at = int(rng.integers(8, bits.size - length))
                gain[at:at + length] = depth
                noise = rng.exponential(0.05, (bits.size, 2))
                powers = noise.copy()
                powers[np.arange(bits.size), bits] += gain
                powers = powers.astype(np.float32)
                soft = np.concatenate([A.soft_bits(p) for p in powers])
                row = np.packbits((soft < 0).astype(np.uint8)).tobytes()
                for i, level in enumerate((0, 16, 32, 64)):
                    if level:
                        got = A.rs_frame_decode(row, 1, C.CRC16, 0x100, erase=A.soft_erasures(soft, level, len(row)))[0]
                    else:
                        got = A.rs_frame_decode(row, 1, C.CRC16, 0x100)[0]
                    lost[i] += bytes(got) != sent
            table.append((length, depth, *lost))
    return table


def test_level_study_is_reported(A, capsys):
    table = level_study(A, trials=6)
    with capsys.disabled():
        print("\nfade symbols, depth, frames lost of 6: errors only, level 16, 32, 64")
        for row in table:
            print("  %4d  %.2f  %2d %2d %2d %2d" % row)
    assert len(table) == 15
