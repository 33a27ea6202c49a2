"""Numpy restatement of the transmitter (include/demod.h "transmitter"): the
reference of tests/test_tx_cpu.py and tests/test_gpu_tx.py, on top of
frames_check_ref / frames_fec_ref (the frame's bytes and symbols). Exact integer
arithmetic: uint32 phases, uint64 counters, int64 noise; the sine table is the
oracle's (oracle.sine_lut()).

send() and modulate() restate the two device stages on arrays laid out as the
device's (the GPU tests lay them over the same poison); Tx is a transmitter of S
streams on such arrays.
"""
import math
from types import SimpleNamespace

import numpy as np

import frames_check_ref as C
import frames_ref as F
import rx_ref as RX

STATE_DTYPE = np.dtype([("head", "<u8"), ("tail", "<u8"), ("accepted", "<u8"), ("refused", "<u8"),
                        ("offset", "<u4"), ("phase", "<u4")])
RECORD_DTYPE = np.dtype([("length", "<u4"), ("body", "<u4")])
PLACE_DTYPE = np.dtype([("start", "<u8"), ("symbols", "<u4"), ("status", "<u4")])
assert STATE_DTYPE.itemsize == 40 and RECORD_DTYPE.itemsize == 8 and PLACE_DTYPE.itemsize == 16
OK, BAD_LENGTH, NO_ROOM = 0, 1, 2
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


def mix64(z):
    """splitmix64's finaliser on a uint64 array (wrapping)."""
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def inc_table(freqs, fs=48000.0):
    """inc[16]: llround(f / fs 2^32) & 0xFFFFFFFF for the K tones, 0 behind them."""
    inc = np.zeros(16, np.uint64)
    for t, f in enumerate(freqs):
        inc[t] = int(math.floor(float(f) / fs * 4294967296.0 + 0.5)) & M32
    return inc


def make(freqs, n, lut, sync, h=2, kind=C.CRC16, fec=0, max_len=16, gap=0, idle=(0,), amplitude=8000,
         sigma=0, seed=0, ring=None, max_frames=4, stride=2880, fs=48000.0):
    """The pair (configuration, transmitter configuration) the reference needs."""
    K = len(freqs)
    c = SimpleNamespace(K=K, n=n, bits=F.bits_per_symbol(K), inc=inc_table(freqs, fs),
                        lut=np.asarray(lut, np.int64), sync=np.asarray(sync, np.uint8), h=h, kind=kind, fec=fec,
                        max_len=max_len, gap=gap, idle=np.asarray(idle, np.uint8), amplitude=amplitude,
                        sigma=sigma, seed=seed, max_frames=max_frames, stride=stride)
    c.C = ring if ring is not None else frame_count(c, max_len) + gap
    return c


def frame_count(c, length):
    """A(length): the word and the payload symbols."""
    return len(c.sync) + RX.span(length, c.bits, c.h, c.kind, c.fec)


def frame_symbols(c, data):
    """The A(len(data)) symbols of one frame on the air."""
    return RX.frame_symbols(bytes(data), c.sync, c.bits, c.h, c.kind, c.fec)


def work_stride(c):
    return (c.n - 1 + c.stride) // c.n + 2


def sizes(c, S):
    """The closed forms of demod_tx_sizes (the caller has checked the refusals)."""
    rows = S * c.max_frames
    return dict(max_symbols=frame_count(c, c.max_len), ring_bytes=S * c.C, state_bytes=40 * S,
                places_bytes=16 * rows, records_bytes=8 * rows, bodies_bytes=rows * c.max_len,
                pcm_bytes=2 * S * c.stride, modulate_work_bytes=4 * S * work_stride(c))


def clamp(c, st):
    """(head, tail, offset) of a stored state, clamped into the invariant."""
    head, offset = int(st["head"]), min(int(st["offset"]), c.n - 1)
    lo, hi = (head + (offset > 0)) & M64, (head + c.C) & M64
    tail = max(min(int(st["tail"]), hi), lo)
    return head, tail, offset


def idle_symbol(c, q):
    return int(c.idle[q % len(c.idle)])


def send(c, state, ring, records, count, data, place_out):
    """demod_tx_encode_async. state STATE_DTYPE [S], ring uint8 [S][C], records
    RECORD_DTYPE [S][max_frames], count uint32 [S], data uint8 [n_bytes], as
    stored. Returns copies (state, ring, place) with what the call writes laid
    over what they held."""
    state, ring, place = state.copy(), ring.copy(), place_out.copy()
    data = np.asarray(data, np.uint8).reshape(-1)
    nb = data.size
    S = len(state)
    for s in range(S):
        head, tail, offset = clamp(c, state[s])
        cnt = min(int(count[s]), c.max_frames)
        e, last, n_acc = 0, 0, 0
        for i in range(cnt):
            ln = int(records["length"][s, i])
            if ln > c.max_len:
                place[s, i] = (0, 0, BAD_LENGTH)
                continue
            A = frame_count(c, ln)
            a = A + c.gap
            e += a
            if tail + e - head > c.C:
                place[s, i] = (0, 0, NO_ROOM)
                continue
            start = tail + e - a
            place[s, i] = (start, A, OK)
            lc = min(ln, nb)
            off = min(int(records["body"][s, i]), nb - lc)
            body = np.zeros(ln, np.uint8)
            body[:lc] = data[off:off + lc]
            sym = np.concatenate([frame_symbols(c, body.tobytes()),
                                  [idle_symbol(c, start + A + j) for j in range(c.gap)]]).astype(np.uint8)
            ring[s, (start + np.arange(a)) % c.C] = sym
            last, n_acc = e, n_acc + 1
        state[s]["head"], state[s]["tail"], state[s]["offset"] = head, (tail + last) & M64, offset
        state[s]["accepted"] = (int(state[s]["accepted"]) + n_acc) & M64
        state[s]["refused"] = (int(state[s]["refused"]) + cnt - n_acc) & M64
    return state, ring, place


def modulate(c, state, ring, count, pcm_out):
    """demod_tx_modulate_async. pcm_out int16 [S][stride]. Returns copies
    (state, ring, pcm) with what the call writes laid over what they held (the
    ring: the idle symbol a pull ends in, mid-symbol, is queued)."""
    state, ring_in, ring, pcm = state.copy(), ring, ring.copy(), pcm_out.copy()
    n = c.n
    for s in range(len(state)):
        head, tail, offset = clamp(c, state[s])
        phase = int(state[s]["phase"])
        m = min(int(count[s]), c.stride)
        y_end = offset + m
        d_end = y_end // n
        n_sym = d_end + 1
        sym = np.array([int(ring_in[s, (head + d) % c.C]) & 15 if head + d < tail else idle_symbol(c, head + d)
                        for d in range(n_sym)], np.int64)
        step = (np.uint64(n) * c.inc[sym]) & np.uint64(M32)
        phi = (np.uint64(phase) + np.concatenate([[0], np.cumsum(step, dtype=np.uint64)]).astype(np.uint64)) \
            & np.uint64(M32)                                   # phi[d] = PHI(head + d), d <= n_sym
        if m:
            y = offset + np.arange(m, dtype=np.uint64)
            d, r = (y // np.uint64(n)).astype(np.int64), y % np.uint64(n)
            ph = (phi[d] + r * c.inc[sym[d]]) & np.uint64(M32)
            tone = (c.amplitude * c.lut[(ph >> np.uint64(18)).astype(np.int64)] + 16384) >> 15
            ns = mix64(np.array([(c.seed + (s + 1) * GAMMA) & M64], np.uint64))[0]
            ctr = np.uint64((head * n + 1) & M64) + y
            z = mix64(ns + ctr * np.uint64(GAMMA))
            f = np.uint64(0xFFFF)
            u = ((z & f) + ((z >> np.uint64(16)) & f) + ((z >> np.uint64(32)) & f) + (z >> np.uint64(48)))
            noise = ((u.astype(np.int64) - 131070) * int(c.sigma) * 113512) >> 32
            pcm[s, :m] = np.clip(tone + noise, -32768, 32767).astype(np.int16)
        head2, off2 = (head + d_end) & M64, y_end % n
        state[s]["head"], state[s]["offset"], state[s]["phase"] = head2, off2, int(phi[d_end])
        if off2 > 0 and head2 >= tail:
            ring[s, head2 % c.C] = idle_symbol(c, head2)
        state[s]["tail"] = max(tail, (head2 + (off2 > 0)) & M64)
    return state, ring, pcm


class Tx:
    """A transmitter of S streams on the device's arrays."""

    def __init__(self, c, S):
        self.c, self.S = c, S
        self.state = np.zeros(S, STATE_DTYPE)
        self.ring = np.zeros((S, c.C), np.uint8)

    def send(self, frames):
        """frames: [(stream, data bytes)] in any stream order. Returns the
        places in input order, or None when the list is refused (more than
        max_frames for one stream, a stream >= S)."""
        c = self.c
        records = np.zeros((self.S, c.max_frames), RECORD_DTYPE)
        count = np.zeros(self.S, np.uint32)
        data, slot = b"", []
        for s, b in frames:
            if s >= self.S or count[s] >= c.max_frames:
                return None
            slot.append((s, int(count[s])))
            records[s, count[s]] = (len(b), len(data) if len(b) <= c.max_len else 0)
            if len(b) <= c.max_len:
                data += bytes(b)
            count[s] += 1
        place = np.zeros((self.S, c.max_frames), PLACE_DTYPE)
        self.state, self.ring, place = send(c, self.state, self.ring, records, count,
                                            np.frombuffer(data, np.uint8), place)
        return np.array([place[s, i] for s, i in slot], PLACE_DTYPE).reshape(-1)

    def pull(self, counts):
        """counts: one per stream (or one for all). Returns the streams' samples."""
        counts = [counts] * self.S if np.isscalar(counts) else list(counts)
        assert max(counts) <= self.c.stride
        pcm = np.zeros((self.S, self.c.stride), np.int16)
        self.state, self.ring, pcm = modulate(self.c, self.state, self.ring, np.asarray(counts, np.uint32), pcm)
        return [pcm[s, :counts[s]].copy() for s in range(self.S)]


# ---- the loopback fixture ------------------------------------------------------------

LOOP_N, LOOP_HOP, LOOP_L, LOOP_H, LOOP_KIND, LOOP_MAX_LEN = 1024, 256, 16, 1, C.CRC16, 3
LOOP_LEAD = 2 * 2880            # samples pulled before the send: it ends mid-symbol, in idle


def loop_tones(K):
    return tuple(1500.0 + 375.0 * i for i in range(K))


def loopback_case(K, fec, lut, n_frames=3):
    """The inputs of the loopback tests (CPU: the reference alone; GPU: the
    handles): amplitude 8000, sigma 400, hop = n / 4, a 16-symbol word, frames
    of 0 .. 3 data bytes with 3 idle symbols behind each, an alternating idle
    pattern. Returns (c, datas, N, total): the transmitter's configuration, the
    frames' data, the receiver's row width in symbols and the samples to pull
    so that the last frame's row is complete."""
    rng = np.random.default_rng(7000 + 10 * K + fec)
    word = rng.integers(0, K, LOOP_L).astype(np.uint8)
    datas = [rng.integers(0, 256, (LOOP_MAX_LEN - f) % (LOOP_MAX_LEN + 1)).astype(np.uint8).tobytes()
             for f in range(n_frames)]
    c = make(loop_tones(K), LOOP_N, lut, word, h=LOOP_H, kind=LOOP_KIND, fec=fec, max_len=LOOP_MAX_LEN, gap=3,
             idle=(0, 1), amplitude=8000, sigma=400, seed=1234 + K, max_frames=n_frames, stride=2880)
    c.C = n_frames * (frame_count(c, LOOP_MAX_LEN) + c.gap) + 5
    N = RX.row_symbols(LOOP_H, LOOP_KIND, fec, c.bits, LOOP_MAX_LEN)
    symbols = -(-LOOP_LEAD // LOOP_N) + sum(frame_count(c, len(d)) + c.gap for d in datas) + N + 6
    total = -(-symbols * LOOP_N // 2880) * 2880
    return c, datas, N, total
