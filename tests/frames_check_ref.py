"""Numpy and Python restatement of the checked frame (include/demod.h "checked
frames"): the reference of tests/test_frames_check_cpu.py and
tests/test_gpu_frames_check.py.

The frame lives on the packed row a frame scan writes (B bytes, MSB first):

  byte 0 .. h-1          len, big-endian, h = len_bytes in {1, 2}
  byte h .. h+len-1      data
  byte h+len .. +c-1     CRC, big-endian, over bytes 0 .. h+len-1
  the rest of the row    ignored

c = 2 (CRC-16/CCITT-FALSE) or 4 (CRC-32/MPEG-2): non-reflected, xorout 0,
bit by bit here. max_len = B - h - c. A frame occupies L + S symbols, S =
ceil((h + len + c) 8 / bits). Per group of rows (ascending windows):

  status    BAD_LENGTH when len > max_len (crc reported as 0), else BAD_CRC
            when the stored CRC differs from the computed one, else OK.
  covered   1 when the row is OK and an OK row before it has end = window +
            (L + S) R (64-bit, wrapping) above the row's window.
  kept      OK and not covered; the kept rows' indices ascending, and their
            data bytes.
  summary   (rows, rows OK, rows kept, 0).

check_group is the one copy of that loop, for the rows of every mode: the
caller hands it S as a function of len (fec_modes_ref.span_of: the coded
modes' and the outer code's spans are other functions of len) and, where the
row is not a plain packed one, the length bound in place of B - h - c.
"""
import numpy as np

CRC16, CRC32 = 1, 2
OK, BAD_LENGTH, BAD_CRC = 0, 1, 2
KINDS = {CRC16: (16, 0x1021, 0xFFFF), CRC32: (32, 0x04C11DB7, 0xFFFFFFFF)}   # width, poly, init
CRC_BYTES = {CRC16: 2, CRC32: 4}
CHECK_DTYPE = np.dtype([("length", "<u4"), ("crc", "<u4"), ("status", "<u4"), ("covered", "<u4")])
SUMMARY_DTYPE = np.dtype([("n_checked", "<u8"), ("n_valid", "<u8"), ("n_kept", "<u8"), ("reserved", "<u8")])
HIT_DTYPE = np.dtype([("window", "<u8"), ("errors", "<u4"), ("reserved", "<u4")])
M64 = (1 << 64) - 1


def crc(kind, data):
    """The CRC of `data`, one bit at a time."""
    width, poly, reg = KINDS[kind]
    top, mask = 1 << (width - 1), (1 << width) - 1
    for byte in bytes(data):
        reg ^= byte << (width - 8)
        for _ in range(8):
            reg = ((reg << 1) ^ poly if reg & top else reg << 1) & mask
    return reg


def encode(data, len_bytes, kind):
    """len || data || CRC, or None where the length does not fit the header or
    is above 4096."""
    data = bytes(data)
    if len(data) > 4096 or len(data) >= 256 ** len_bytes:
        return None
    head = len(data).to_bytes(len_bytes, "big") + data
    return head + crc(kind, head).to_bytes(CRC_BYTES[kind], "big")


def frame_symbols(n_bytes, bits):
    """Symbols that n_bytes bytes occupy."""
    return (n_bytes * 8 + bits - 1) // bits


def unpack(data, n, bits):
    """The first n symbols of `bits` bits in `data`, MSB first (missing bits 0)."""
    b = np.unpackbits(np.frombuffer(bytes(data), np.uint8))
    b = np.concatenate([b, np.zeros(max(0, n * bits - b.size), np.uint8)])[:n * bits].reshape(n, bits)
    return (b << np.arange(bits - 1, -1, -1, dtype=np.uint8)).sum(axis=1).astype(np.uint8)


def pack(symbols, bits):
    """One row of symbols -> bytes: each symbol's low `bits` bits, MSB first, pad bits 0."""
    s = np.asarray(symbols, np.uint8).reshape(-1)
    b = np.unpackbits(s[:, None], axis=1)[:, 8 - bits:].reshape(-1)
    return np.packbits(np.concatenate([b, np.zeros(-b.size % 8, np.uint8)])).tobytes()


def payload_row(frame, N, bits, rng, K=None):
    """A frame's bytes as symbols, padded to N payload symbols with seeded
    random symbols below K (default 2^bits)."""
    S = frame_symbols(len(frame), bits)
    assert S <= N
    row = rng.integers(0, K or (1 << bits), N).astype(np.uint8)
    row[:S] = unpack(frame, S, bits)
    return row


def check_row(row, len_bytes, kind, most=None):
    """(length, crc, status) of one row; `most` is the length bound, None for
    a packed row's own len(row) - len_bytes - c."""
    row = bytes(row)
    c = CRC_BYTES[kind]
    if most is None:
        most = len(row) - len_bytes - c
    assert most >= 0
    length = int.from_bytes(row[:len_bytes], "big")
    if length > most:
        return length, 0, BAD_LENGTH
    n = len_bytes + length
    got = crc(kind, row[:n])
    return length, got, OK if got == int.from_bytes(row[n:n + c], "big") else BAD_CRC


def check_group(windows, rows, L, R, span, most, h, kind):
    """One group's rows (windows [nw], rows uint8 [nw][W]): the one copy of the
    loop. span(length) gives the symbols a frame of `length` data bytes
    occupies behind its word (fec_modes_ref.span_of a mode); `most` is
    check_row's. Returns (check CHECK_DTYPE [nw], kept uint32 [n_kept], bodies:
    the kept rows' data bytes, summary SUMMARY_DTYPE scalar)."""
    nw = len(windows)
    check = np.zeros(nw, CHECK_DTYPE)
    kept, bodies = [], []
    reach = 0          # max end over the OK rows so far
    for i in range(nw):
        length, got, status = check_row(rows[i], h, kind, most)
        covered = 0
        if status == OK:
            w = int(windows[i])
            covered = int(reach > w)
            reach = max(reach, (w + (L + span(length)) * R) & M64)
            if not covered:
                kept.append(i)
                bodies.append(bytes(rows[i][h:h + length]))
        check[i] = (length, got, status, covered)
    summary = np.zeros((), SUMMARY_DTYPE)
    summary["n_checked"], summary["n_valid"] = nw, int((check["status"] == OK).sum())
    summary["n_kept"] = len(kept)
    return check, np.array(kept, np.uint32), bodies, summary


def check_groups(hits, rows, n_written, max_frames, L, R, span, most, h, kind):
    """hits HIT_DTYPE [G][max_frames], rows uint8 [G][max_frames][W], n_written
    [G] as stored (clamped to max_frames here). One check_group result per
    group."""
    out = []
    for g, n in enumerate(n_written):
        nw = min(int(n), max_frames)
        out.append(check_group(hits[g]["window"][:nw], rows[g][:nw], L, R, span, most, h, kind))
    return out
