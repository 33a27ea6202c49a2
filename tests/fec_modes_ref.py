"""Numpy restatement of the coded modes (include/demod.h "punctured and
interleaved"): the reference of tests/test_fec_modes_cpu.py and
tests/test_gpu_fec_modes.py. Nothing here calls the library.

A mode is 1 | {0, 0x10 (rate 2/3), 0x20 (rate 3/4)} | {0, 0x40 (interleaved)}.
Mother bit m = 2 t + v of the rate-1/2 code 0171/0133 is kept or punctured by
the phase of its step; a kept bit's code index is i = Nt(t) + its rank among
step t's kept bits; with the interleaver code index r 16 + c of each block of
256 sits at air position c 16 + r.

A mode is decoded by re-ordering the air soft values into a rate-1/2 trellis
array of 2 St values, zeros at the punctured positions, and handing that to
the existing tests/frames_fec_ref.py decoder: the decoder the earlier tests
hold to a maximum-likelihood reference is the oracle here too.

span, row_shape and symbols_for take any `fec` the stages take: 0 or a mode in
the low byte, with or without a parity flag of the outer code (tests/rs_ref.py).
They are the one span, row shape and row size of the check references, of
tests/rx_ref.py and of tests/rs_chain_ref.py.
"""
import functools

import numpy as np

import frames_check_ref as C
import frames_fec_ref as X
import rs_ref as R

CONV_K7, RATE_2_3, RATE_3_4, INTERLEAVE = 1, 0x10, 0x20, 0x40
BLOCK = 256
MODES = (0x01, 0x11, 0x21, 0x41, 0x51, 0x61)
NEW_MODES = MODES[1:]
BAD_MODES = (2, 0x10, 0x31, 0x81)
# the mother bits v kept at each step phase
KEEP = {0: ((0, 1),), RATE_2_3: ((0, 1), (1,)), RATE_3_4: ((0, 1), (0,), (1,))}


def pattern(fec):
    return KEEP[fec & 0x30]


@functools.lru_cache(maxsize=None)
def kept_bits(fec, T):
    """Nt(T), by counting (each (mode, T) once: the receiver's reference asks per row)."""
    pat = pattern(fec)
    return sum(len(pat[t % len(pat)]) for t in range(T))


def steps_within(fec, Cu):
    """St: the greatest T with Nt(T) <= Cu, by stepping."""
    pat, T, n = pattern(fec), 0, 0
    while n + len(pat[T % len(pat)]) <= Cu:
        n += len(pat[T % len(pat)])
        T += 1
    return T


def interleave(fec, i):
    if not fec & INTERLEAVE:
        return i
    blk, r, c = i // BLOCK, (i % BLOCK) // 16, i % 16
    return blk * BLOCK + c * 16 + r


def air_map(fec, T):
    """int64 [2 T]: the air position of each mother bit of T steps, -1 where punctured."""
    pat = pattern(fec)
    out = np.full(2 * T, -1, np.int64)
    i = 0
    for t in range(T):
        for v in pat[t % len(pat)]:
            out[2 * t + v] = interleave(fec, i)
            i += 1
    return out


def air_bits(fec, T):
    """Na: Nt(T), rounded up to whole blocks with the interleaver."""
    n = kept_bits(fec, T)
    return -(-n // BLOCK) * BLOCK if fec & INTERLEAVE else n


def span(length, bits, h, kind, fec):
    """The symbols a frame of `length` data bytes occupies behind its word, in
    every mode: fec's low byte 0 or one of MODES, with or without a parity flag
    of the outer code (rs_ref). Its n' bytes' bits; with the convolutional code
    the Na air bits of its T = max(8 n' + 6, 8 h + 64) steps."""
    n = R.frame_size(h + length + C.CRC_BYTES[kind], R.mode_parity(fec))
    conv = fec & 0xFF
    air = air_bits(conv, max(8 * n + 6, 8 * h + X.DEPTH)) if conv else 8 * n
    return -(-air // bits)


def span_of(bits, h, kind, fec):
    """span of the mode as a function of the length: what frames_check_ref.check_group takes."""
    return lambda length: span(length, bits, h, kind, fec)


def encode_air(info, T, fec):
    """The Na air bits of the information bytes `info` over T steps, one per element."""
    mother = X.encode_bits(info, T)
    amap = air_map(fec, T)
    out = np.zeros(air_bits(fec, T), np.uint8)
    out[amap[amap >= 0]] = mother[amap >= 0]
    return out


def encode(data, h, kind, fec):
    """The frame's bytes in air order, or None where the checked frame is refused."""
    frame = C.encode(data, h, kind)
    if frame is None:
        return None
    return np.packbits(encode_air(frame, X.steps(len(data), h, kind), fec)).tobytes()


def row_shape(N, bits, h, kind, fec):
    """(St, W, max_len) of rows of N symbols, or None where the row is refused:
    W = B packed bytes and St = 0 without the convolutional code, else St steps
    that decode to W = Bd bytes; max_len the greatest len whose n' fits W."""
    Cc, conv = N * bits, fec & 0xFF
    St, W = 0, (Cc + 7) // 8
    if conv:
        St = steps_within(conv, Cc // BLOCK * BLOCK if conv & INTERLEAVE else Cc)
        if St < 8 * h + X.DEPTH:
            return None
        W = (St - 6) // 8
    max_len = R.max_len(W, h, C.CRC_BYTES[kind], R.mode_parity(fec))
    if max_len < 0 or max_len > 4096:
        return None
    return St, W, max_len


def symbols_for(most, bits, h, kind, fec):
    """The smallest N whose rows hold frames of `most` data bytes and all their
    symbols. Where no row does (near the payload limit a row that holds `most`
    can hold more than 4096 and is refused) that is an error, not a search
    without end: a fitting row lies within two blocks and a byte of the span."""
    first = span(most, bits, h, kind, fec)
    for N in range(first, first + 2 * BLOCK + 8):
        shape = row_shape(N, bits, h, kind, fec)
        if shape is not None and shape[2] >= most:
            return N
    raise ValueError("no row of the mode holds frames of %d data bytes" % most)


def trellis_soft(soft, fec):
    """Air-order soft values int8 [.., C] -> the rate-1/2 trellis array int8 [.., 2 St]."""
    soft = np.asarray(soft, np.int8)
    Cc = soft.shape[-1]
    St = steps_within(fec, Cc // BLOCK * BLOCK if fec & INTERLEAVE else Cc)
    amap = air_map(fec, St)
    out = np.zeros(soft.shape[:-1] + (2 * St,), np.int8)
    out[..., amap >= 0] = soft[..., amap[amap >= 0]]
    return out


def decode_rows(soft, h, kind, fec):
    """soft int8 [n][C] in air order: frames_fec_ref.decode_rows of the trellis array."""
    return X.decode_rows(trellis_soft(soft, fec), h, kind)


def decode(soft, h, kind, fec):
    """One row: (the bytes written, its DECODE_DTYPE record)."""
    return X.decode(trellis_soft(soft, fec), h, kind)


def edge_lengths(max_len, h, kind, fec):
    """0, 1, either side of 8 n + 6 = 8 h + 64, max_len, and the lengths whose
    Nt(T) is 255, 256 and 257 mod 256: the first length up to max_len that hits
    each residue, or where the mode's Nt never does (2 T = 16 n + 12 cannot)
    the first that comes nearest to it."""
    c = C.CRC_BYTES[kind]
    out = {n for n in (0, 1, 7 - c, 8 - c, max_len) if 0 <= n <= max_len}
    res = [kept_bits(fec, X.steps(n, h, kind)) % BLOCK for n in range(max_len + 1)]
    for want in (255, 0, 1):
        out.add(min(range(max_len + 1), key=lambda n: min((res[n] - want) % BLOCK, (want - res[n]) % BLOCK)))
    return sorted(out)
