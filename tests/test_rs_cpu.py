"""The Reed-Solomon outer code on the host (include/demod.h "Reed-Solomon
outer code"): the pinned vectors, the encoder and the decoder
demod_rs_frame_decode against the independent reference tests/rs_ref.py
(another algorithm) and its decoder-free checker, the layout against a
brute-force count, the 20 modes and the refusals at every host entry that
takes `fec`, two link statements through the host chain alone, and the host
sources in a stand-alone program under AddressSanitizer and UBSan
(tests/native/rs_host_test.c).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fec_modes_ref as Z
import frames_check_ref as C
import rs_cases as RC
import rs_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS, FLAGS, BAD_MODES, PATTERNS = RC.KINDS, RC.FLAGS, RC.BAD_MODES, RC.PATTERNS
edge_lengths, corrupt = RC.edge_lengths, RC.corrupt


def test_exports_and_constants(A):
    lib = A.load_library()
    for name in ("demod_rs_generator", "demod_rs_encode", "demod_rs_frame_size", "demod_rs_max_len",
                 "demod_rs_frame_encode", "demod_rs_frame_decode", "demod_frames_rs_async"):
        assert hasattr(lib, name), name
        assert name in A.header_exports()
    assert (A.DEMOD_FEC_RS16, A.DEMOD_FEC_RS32) == FLAGS
    assert (A.DEMOD_RS_OK, A.DEMOD_RS_BAD_LENGTH, A.DEMOD_RS_FAILED) == (R.OK, R.BAD_LENGTH, R.FAILED)
    assert ctypes.sizeof(A.DemodFrameRs) == 16 and A.FRAME_RS_DTYPE.names == ("status", "codewords", "corrected",
                                                                              "failed")
    assert len(A.RS_MODES) == 20 and len(set(A.RS_MODES)) == 20 and 0 not in A.RS_MODES
    assert set(A.RS_MODES) == {m | r for m in (0,) + tuple(A.FEC_MODES) for r in (0,) + FLAGS} - {0}


def test_pins(A):
    """The QR-code vector (P = 10), g of P = 16 and the parity of "123456789",
    from the library and from the reference."""
    msg = bytes.fromhex("205B0B78D172DC4D4340EC11EC11EC11")
    g16 = bytes.fromhex("013B0D68BD44D11E08A34129E56232243B")
    p16 = bytes.fromhex("5755a770f1f69c34920d6386a4191a96")
    p32 = bytes.fromhex("4efff55efc5f5351284fef58773aaabfda9ee07e544dd23587cd189fc338daca")
    qr = bytes.fromhex("C4232777EBD7E7E25D17")
    assert A.rs_encode(msg, 10) == qr == bytes(R.parity(msg, 10))
    assert A.rs_generator(16) == g16 == bytes(R.generator(16))
    assert A.rs_encode(b"123456789", 16) == p16 == bytes(R.parity(b"123456789", 16))
    assert A.rs_encode(b"123456789", 32) == p32 == bytes(R.parity(b"123456789", 32))
    assert A.rs_generator(32) == bytes(R.generator(32))
    for bad in (lambda: A.rs_encode(msg, 0), lambda: A.rs_encode(msg, 33), lambda: A.rs_encode(b"", 16),
                lambda: A.rs_encode(bytes(240), 16), lambda: A.rs_generator(0), lambda: A.rs_generator(33)):
        with pytest.raises(A.DemodError):
            bad()


# ---- the layout ---------------------------------------------------------------------

@pytest.mark.parametrize("flag", FLAGS)
def test_layout_against_a_count(A, flag):
    """n'(len) and max_len(W) against rs_ref's counted ones; the payload-limit
    figures of the header."""
    P = R.PARITY[flag]
    assert A.rs_frame_size(4096, 2, C.CRC32, flag) == {16: 4390, 32: 4710}[P]
    assert R.codewords(4102, P) == {16: 18, 32: 19}[P]
    for h in (1, 2):
        for kind in KINDS:
            c = C.CRC_BYTES[kind]
            top = 255 if h == 1 else 4096
            sizes = [A.rs_frame_size(n, h, kind, flag) for n in range(top + 1)]
            assert sizes == [R.frame_size(h + n + c, P) for n in range(top + 1)]
            assert all(b > a for a, b in zip(sizes, sizes[1:])), "n' increases strictly"
            with pytest.raises(A.DemodError):
                A.rs_frame_size(top + 1, h, kind, flag)
            # every width up to three codewords, then the widths around the payload limit
            first = R.frame_size(h + c, P)
            for W in list(range(0, 3 * 255 + 8)) + list(range(4380, 4720, 7)):
                want = R.max_len(W, h, c, P)
                if want < 0:
                    assert W < first
                    with pytest.raises(A.DemodError):
                        A.rs_max_len(W, h, kind, flag)
                else:
                    assert A.rs_max_len(W, h, kind, flag) == want, (W, h, kind)
            # without a parity flag the frame is the checked frame
            assert A.rs_frame_size(10, h, kind, 1) == h + 10 + c and A.rs_max_len(40, h, kind, 0x41) == 40 - h - c


def test_reference_span_equals_the_library(A):
    """fec_modes_ref.span, the span every check reference and the receiver's
    reference use, against demod_fec_frame_symbols and against
    demod_tx_frame_symbol_count less the word: every mode, bits 1 to 4, both
    header sizes and CRC kinds, at the lengths where the outer code's layout
    changes and where the convolutional modes' kept bits cross a block.
    demod_fec_frame_symbols refuses a mode without the convolutional code."""
    word, n = (1, 0, 1), 0
    for fec in A.RS_MODES:
        conv = fec & 0xFF
        for h in (1, 2):
            for kind in KINDS:
                c = C.CRC_BYTES[kind]
                lens = set(Z.edge_lengths(255 if h == 1 else 600, h, kind, conv or Z.CONV_K7))
                for P in R.PARITY.values():
                    lens.update(edge_lengths(h, c, P))
                tx = A.make_tx_cfg(word, h, kind, fec, 4096)
                for length in sorted(lens):
                    for bits in (1, 2, 3, 4):
                        want = Z.span(length, bits, h, kind, fec)
                        what = (fec, h, kind, length, bits)
                        assert A.tx_frame_symbol_count(tx, 1 << bits, length) - len(word) == want, what
                        if conv:
                            assert A.fec_frame_symbols(length, h, kind, bits, fec) == want, what
                        else:
                            with pytest.raises(A.DemodError):
                                A.fec_frame_symbols(length, h, kind, bits, fec)
                        n += 1
    assert n > 20 * 2 * 2 * 4 * 8


# ---- encoder and decoder against the reference -----------------------------------------

@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("h", (1, 2))
def test_encoder_and_decoder_against_the_reference(A, flag, h):
    P, t = R.PARITY[flag], R.PARITY[flag] // 2
    rng = np.random.default_rng(100 * h + P)
    for kind in KINDS:
        c = C.CRC_BYTES[kind]
        for length in edge_lengths(h, c, P):
            data = bytes(rng.integers(0, 256, length, dtype=np.uint8))
            sent = A.rs_frame_encode(data, h, kind, flag)
            assert sent == R.frame_encode(data, h, kind, P), (length, kind)
            n = h + length + c
            for pattern in PATTERNS:
                # W = n' + 5; at the payload limit W = n', as a wider row is refused
                row = bytearray(sent + bytes(rng.integers(0, 256, 0 if length == 4096 else 5, dtype=np.uint8)))
                corrupt(row, n, P, h, pattern, rng)
                got, rec, covered = A.rs_frame_decode(bytes(row), h, kind, flag)
                want, wrec = R.frame_decode(bytes(row), h, kind, P)
                assert bytes(got) == want and rec == wrec, (length, kind, pattern, rec, wrec)
                R.check_frame(bytes(row), bytes(got), rec, h, kind, P)
                if pattern == "header":
                    continue   # detected, not repaired: whatever the outcome, it equals the reference
                assert covered == len(sent)
                if pattern != "t+1":
                    assert bytes(got[:len(sent)]) == sent and rec["status"] == R.OK, (length, kind, pattern)
                    assert rec["corrected"] == {"none": 0, "one": 1, "t": t, "parity": t, "ends": 2}[pattern] * \
                        rec["codewords"]
                else:
                    assert bytes(got[:len(sent)]) != sent   # t + 1 away: never the frame that was sent


def test_bad_length_reads_nothing_past_the_header(A):
    for flag in FLAGS:
        row = bytes([200]) + bytes(range(60))            # W = 61: max_len is far below 200
        got, rec, covered = A.rs_frame_decode(row, 1, C.CRC16, flag)
        assert bytes(got) == row and covered == 1
        assert rec == dict(status=R.BAD_LENGTH, codewords=0, corrected=0, failed=0)
        assert R.frame_decode(row, 1, C.CRC16, R.PARITY[flag])[1] == rec


# ---- the modes ----------------------------------------------------------------------------

def test_modes_at_every_host_entry(A):
    """The 20 modes are accepted and 0, 2, 0x10, 0x31 and 0x81 (and both
    parity flags together) refused by every host entry that takes fec."""
    lib = A.load_library()
    cfg2 = A.make_cfg(n=1024, hop=256, freqs=A.FSK2_FREQS)
    word = [0, 1, 1, 0, 1]
    rx_base = dict(sync=word, max_errors=0, frame_symbols=1024, len_bytes=1, crc=C.CRC16, max_frames=4,
                   ring_windows=2 * 1029 * 4)
    tx_base = dict(sync=word, len_bytes=1, crc=C.CRC16, max_len=16, ring_symbols=8192)
    soft = np.zeros(1024, np.int8)
    for fec in A.RS_MODES:
        conv, P = fec & 0xFF, R.mode_parity(fec)
        n = R.frame_size(1 + 16 + 2, P)
        assert A.rs_frame_size(16, 1, C.CRC16, fec) == n
        assert len(A.rs_frame_encode(bytes(16), 1, C.CRC16, fec)) == n
        assert A.rs_max_len(n, 1, C.CRC16, fec) == 16
        assert A.rs_frame_decode(A.rs_frame_encode(bytes(16), 1, C.CRC16, fec), 1, C.CRC16, fec)[1]["status"] == 0
        z = A.rx_sizes(cfg2, A.make_rx_cfg(fec=fec, **rx_base), 2)
        W = A.fec_row_bytes(1024, 1, 1, conv) if conv else 128
        assert z["row_bytes"] == W and z["max_len"] == R.max_len(W, 1, 2, P)
        assert z["bodies_bytes"] == 2 * 4 * z["max_len"] and (z["decode_work_bytes"] > 0) == bool(conv)
        tz = A.tx_sizes(cfg2, A.make_tx_cfg(fec=fec, **tx_base), 2)
        sym = A.tx_frame_symbols(A.make_tx_cfg(fec=fec, **tx_base), 2, bytes(16))
        assert tz["max_symbols"] == len(sym)
        if conv:
            assert A.fec_frame_symbols(16, 1, C.CRC16, 1, fec) == len(sym) - 5
            assert A.fec_row_bytes(1024, 1, 1, fec) == W and A.fec_air_index(fec, 0) == A.fec_air_index(conv, 0)
            assert A.fec_decode_workspace_size(cfg2, 2, 4, 1024, fec) == z["decode_work_bytes"]
            air = A.fec_frame_encode(bytes(16), 1, C.CRC16, fec)
            assert np.array_equal(A.unpack_symbols(air, len(sym) - 5, 1), sym[5:])
            A.fec_frame_decode(soft, 1, C.CRC16, fec)
        else:
            assert len(sym) == 5 + 8 * n
            packed = A.rs_frame_encode(bytes(16), 1, C.CRC16, fec)
            assert np.array_equal(A.unpack_symbols(packed, 8 * n, 1), sym[5:])
            for call in (lambda: A.fec_frame_symbols(16, 1, C.CRC16, 1, fec), lambda: A.fec_air_index(fec, 0),
                         lambda: A.fec_frame_encode(b"", 1, C.CRC16, fec), lambda: A.fec_row_bytes(1024, 1, 1, fec),
                         lambda: A.fec_frame_decode(soft, 1, C.CRC16, fec),
                         lambda: A.fec_decode_workspace_size(cfg2, 2, 4, 1024, fec)):
                with pytest.raises(A.DemodError):   # the trellis's functions need the convolutional code
                    call()
    out = (ctypes.c_uint8 * 64)()
    rec = A.DemodFrameRs()
    for fec in BAD_MODES + (0x300, 0x301, 0x400):
        assert lib.demod_rs_frame_size(0, 1, C.CRC16, fec) == A.DEMOD_BAD_ARG
        assert lib.demod_rs_max_len(64, 1, C.CRC16, fec) == A.DEMOD_BAD_ARG
        assert lib.demod_rs_frame_encode(None, 0, 1, C.CRC16, fec, out, 64) == A.DEMOD_BAD_ARG
        assert lib.demod_rs_frame_decode(out, 64, 1, C.CRC16, fec, ctypes.byref(rec)) == A.DEMOD_BAD_ARG
        assert lib.demod_fec_frame_symbols(0, 1, C.CRC16, 1, fec) == A.DEMOD_BAD_ARG
        assert lib.demod_fec_air_index(fec, 0) == A.DEMOD_BAD_ARG
        assert lib.demod_fec_row_bytes(1024, 1, 1, fec) == A.DEMOD_BAD_ARG
        assert lib.demod_fec_decode_workspace_size(ctypes.byref(cfg2), 1, 4, 1024, fec) == 0
        if fec:   # 0 is "no code" to the receiver and the transmitter, as before
            with pytest.raises(A.DemodError):
                A.rx_sizes(cfg2, A.make_rx_cfg(fec=fec, **rx_base), 2)
            with pytest.raises(A.DemodError):
                A.tx_sizes(cfg2, A.make_tx_cfg(fec=fec, **tx_base), 2)
            with pytest.raises(A.DemodError):
                A.tx_frame_symbols(A.make_tx_cfg(fec=fec, **tx_base), 2, b"ab")
        d = object.__new__(A.Demodulator)   # the mirror's device entries judge fec before any tensor
        d._lib, d.cfg, d._h = lib, cfg2, None
        for call in (lambda: d.frames_rs_async(None, None, 1, 4, 1024, 1, C.CRC16, fec, None),
                     lambda: d.frames_check_coded_async(None, None, None, 1, 4, 5, 1024, 1, C.CRC16, None, None, None,
                                                        None, fec=fec),
                     lambda: d.frames_coded(np.zeros(8192, np.int16), word, frame_symbols=1024, fec=fec)):
            with pytest.raises(A.DemodError) as e:
                call()
            assert "fec" in str(e.value)
    d = object.__new__(A.Demodulator)
    d._lib, d.cfg, d._h = lib, cfg2, None
    for fec in A.FEC_MODES:   # the stage refuses a mode without a parity flag
        with pytest.raises(A.DemodError) as e:
            d.frames_rs_async(None, None, 1, 4, 1024, 1, C.CRC16, fec, None)
        assert "parity" in str(e.value)
    # rows narrower than the shortest protected frame, and wider than the payload limit allows
    with pytest.raises(A.DemodError):
        A.rx_sizes(cfg2, A.make_rx_cfg(fec=0x100, **dict(rx_base, frame_symbols=8 * 18, ring_windows=4096)), 2)
    A.rx_sizes(cfg2, A.make_rx_cfg(fec=0x100, **dict(rx_base, frame_symbols=8 * 19, ring_windows=4096)), 2)
    wide = dict(rx_base, len_bytes=2, ring_windows=2 * (5 + 8 * 4389) * 4)
    assert A.rx_sizes(cfg2, A.make_rx_cfg(fec=0x100, **dict(wide, frame_symbols=8 * 4388)), 1)["max_len"] == 4096
    with pytest.raises(A.DemodError):
        A.rx_sizes(cfg2, A.make_rx_cfg(fec=0x100, **dict(wide, frame_symbols=8 * 4389)), 1)


# ---- two link statements, through the host chain alone ---------------------------------------

def crc_ok(A, row, h, kind):
    """The check's verdict on a row: (OK, the data bytes)."""
    c = C.CRC_BYTES[kind]
    length = int.from_bytes(row[:h], "big")
    if h + length + c > len(row):
        return False, b""
    stored = int.from_bytes(row[h + length:h + length + c], "big")
    return A.crc(kind, bytes(row[:h + length])) == stored, bytes(row[h:h + length])


def test_link_plain_eight_wrong_bytes(A):
    """fec = 0x100: a frame with 8 wrong bytes comes back; the same wrong
    symbols at fec = 0 lose the frame."""
    rng = np.random.default_rng(11)
    data = bytes(rng.integers(0, 256, 120, dtype=np.uint8))
    frame = A.rs_frame_encode(data, 1, C.CRC16, 0x100)
    sym = A.unpack_symbols(frame, 8 * len(frame), 1)
    plain = A.checked_frame_encode(data, 1, C.CRC16)
    assert frame[:len(plain)] == plain            # the same symbols on the air, then the parity
    wrong = rng.choice(np.arange(1, len(plain)), 8, replace=False)
    for b in wrong:
        sym[8 * b + int(rng.integers(8))] ^= 1      # one wrongly decided symbol in each of 8 bytes
    row = A.pack_symbols(sym, 1)
    got, rec, _ = A.rs_frame_decode(row, 1, C.CRC16, 0x100)
    assert rec == dict(status=R.OK, codewords=1, corrected=8, failed=0)
    assert crc_ok(A, bytes(got), 1, C.CRC16) == (True, data)
    assert crc_ok(A, row[:len(plain)], 1, C.CRC16)[0] is False


def test_link_coded_burst(A):
    """fec = 0x101 against fec = 1: a burst of inverted coded bits at a fixed
    place. The shortest burst that loses the frame at fec = 1 is found by a
    search over lengths; the same burst at fec = 0x101 comes back."""
    rng = np.random.default_rng(12)
    data = bytes(rng.integers(0, 256, 96, dtype=np.uint8))
    start = 500

    def run(fec, burst):
        air = A.fec_frame_encode(data, 1, C.CRC16, fec)
        S = A.fec_frame_symbols(len(data), 1, C.CRC16, 1, fec)
        bits = np.unpackbits(np.frombuffer(air, np.uint8))[:S]
        soft = np.concatenate([np.where(bits == 1, -127, 127), np.zeros(64)]).astype(np.int8)
        soft[start:start + burst] *= -1
        row, dec = A.fec_frame_decode(soft, 1, C.CRC16, fec)
        assert dec["status"] == A.DEMOD_DECODE_OK and dec["length"] == len(data)
        rec = None
        if fec & 0x300:
            assert len(row) >= A.rs_frame_size(len(data), 1, C.CRC16, fec)
            row, rec, _ = A.rs_frame_decode(row, 1, C.CRC16, fec)
        return crc_ok(A, bytes(row), 1, C.CRC16) == (True, data), rec

    assert run(1, 0)[0] and run(0x101, 0) == (True, dict(status=R.OK, codewords=1, corrected=0, failed=0))
    lost = next((b for b in range(1, 65) if not run(1, b)[0]), None)
    # free distance 10: a wrong path wins only with at least 5 of its 10 differing bits inverted
    assert lost is not None and lost >= 5, lost
    back, rec = run(0x101, lost)
    assert back and rec["status"] == R.OK and 1 <= rec["corrected"] <= 8, (lost, rec)


# ---- the host sources under sanitizers -----------------------------------------------------------

def test_standalone_program_under_sanitizers(tmp_path):
    """tests/native/rs_host_test.c with the host sources, built with
    -fsanitize=address,undefined and run as a program of its own."""
    csrc = os.path.join(ROOT, "audio-network_amd", "csrc")
    exe = str(tmp_path / "rs_host_test")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "native", "rs_host_test.c"), os.path.join(csrc, "demod_rs.c"),
                    os.path.join(csrc, "demod_fec.c"), os.path.join(csrc, "demod_tx_frame.c"),
                    os.path.join(csrc, "demod_frame_check.c"), os.path.join(csrc, "demod_frame.c"), "-lm",
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "rs_host_test OK" in r.stdout
