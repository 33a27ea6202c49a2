"""Numpy restatement of the receiver (include/demod.h "receiver"): the reference
of tests/test_rx_cpu.py and tests/test_gpu_rx.py, composed from
frames_segments_ref (the scan of X as one segment), frames_check_ref (the
check of a group's rows), frames_fec_ref (soft values) and fec_modes_ref (row
shape, decode and span of every mode; mode 1 is the rate-1/2 code).

fec is 0 or a coded mode (fec_modes_ref.MODES) everywhere: span(), sizes(),
row_symbols() and scan_check() are the one place that turns it into a span, a
row shape or a decode, and collect(), Rx and one_shot() go through them.

Per stream a run X of detector outputs, sym[i] and P[i][K], i < fill, window i
being the stream's window base + i; with it keep, hold, dropped, cut_hits, all
0 at first. A push with `new` fresh windows:

  1 advance  keep' = min(keep, fill); Y = X[keep':] + new; base += keep'; the
             oldest d = max(len(Y) - C, 0) windows go (base += d, dropped += d).
  2 scan     X as segment {0, fill}; plain: packed rows and check_group; coded:
             soft values of X, decode_rows, the coded check_group.
  3 collect  end_j = base + window_j + (L + S_j) R over the OK rows; a kept row
             is emitted when base + window >= hold (hold from the pushes
             before); then hold = max(hold, max end_j); keep = max(0, t - (R -
             1)), t = tail_window if >= 0 else fill - (L - 1) R; cut_hits +=
             n_hits - n_written.
  4 output   stream 0's emitted rows, then stream 1's, ..; body = the exclusive
             prefix of the lengths in that order.

Three layers, each usable alone: advance() and collect() restate the two device
stages on arrays laid out as the device's (the GPU tests lay them over the same
poison); Rx is the whole receiver over (sym, P) pieces; one_shot() is
demod_frames_checked / demod_frames_coded's kept frames on a whole recording.
"""
import numpy as np

import acquire_ref
import fec_modes_ref as Z
import frames_check_ref as C
import frames_fec_ref as FEC
import frames_ref as F
import frames_segments_ref as FS

FRAME_DTYPE = np.dtype([("stream", "<u4"), ("length", "<u4"), ("window", "<u8"), ("body", "<u8"),
                        ("errors", "<u4"), ("reserved", "<u4")])
STATE_DTYPE = np.dtype([("base", "<u8"), ("hold", "<u8"), ("dropped", "<u8"), ("cut_hits", "<u8"),
                        ("fill", "<u4"), ("keep", "<u4")])
SUMMARY_DTYPE = np.dtype([("n_frames", "<u8"), ("n_bytes", "<u8"), ("n_checked", "<u8"), ("n_valid", "<u8")])
RESULT_DTYPE = F.RESULT_DTYPE          # demod_frames_result_t
M64 = C.M64
assert FRAME_DTYPE.itemsize == 32 and STATE_DTYPE.itemsize == 40 and SUMMARY_DTYPE.itemsize == 32


span = Z.span          # S: the symbols a frame of `length` data bytes occupies behind its word


def min_ring(L, N, R):
    return 2 * (L + N) * R


def collect_work_bytes(S):
    """demod_rx_collect_workspace_size: two 8-byte words and one 4-byte word per
    stream, the last array rounded up to 8."""
    return 16 * S + (4 * S + 7) // 8 * 8


def sizes(K, R, S, L, N, h, kind, fec, max_frames, ring):
    """The closed forms of demod_rx_sizes (the caller has checked the refusals)."""
    bits = F.bits_per_symbol(K)
    c = C.CRC_BYTES[kind]
    if fec:
        St, B, max_len = Z.row_shape(N, bits, h, kind, fec)
        waves = min(max_frames, max(16384 // S, 1))
        decode = S * waves * St * 8
    else:
        B = (N * bits + 7) // 8
        max_len, decode = B - h - c, 0
    rows = S * max_frames
    return dict(max_len=max_len, row_bytes=B, ring_sym_bytes=S * ring, ring_mag_bytes=S * ring * K * 4,
                scan_work_bytes=FS.workspace_size(R, S, S * ring), decode_work_bytes=decode,
                collect_work_bytes=collect_work_bytes(S), frames_bytes=rows * 32, bodies_bytes=rows * max_len)


# ---- the device stages on the device's arrays -----------------------------------

def advance(state, ring_sym_in, ring_mag_in, new_sym, new_mag, new_first, new_count, ring_sym_out,
            ring_mag_out, first_out, count_out):
    """demod_rx_advance_async. state STATE_DTYPE [S]; rings [S][C] and
    [S][C][K] (any 4-byte dtype: the powers are moved, not computed with); the
    new batch [W], [W][K]; the tables as stored. Returns copies (state, ring_sym,
    ring_mag, first, count) of the outputs with what the call writes laid over
    what they held."""
    state = state.copy()
    sym, mag = ring_sym_out.copy(), ring_mag_out.copy()
    first, count = first_out.copy(), count_out.copy()
    S, Cw = ring_sym_in.shape
    W = len(new_sym)
    for s in range(S):
        fill = min(int(state["fill"][s]), Cw)
        keep = min(int(state["keep"][s]), fill)
        f, c = FS.SR.clamp(new_first[s], new_count[s], W)
        ys = np.concatenate([ring_sym_in[s, keep:fill], new_sym[f:f + c]])
        ym = np.concatenate([ring_mag_in[s, keep:fill], new_mag[f:f + c]])
        d = max(len(ys) - Cw, 0)
        ys, ym = ys[d:], ym[d:]
        sym[s, :len(ys)], mag[s, :len(ys)] = ys, ym
        state["base"][s] = (int(state["base"][s]) + keep + d) & M64
        state["dropped"][s] = (int(state["dropped"][s]) + d) & M64
        state["fill"][s], state["keep"][s] = len(ys), 0
        first[s], count[s] = s * Cw, len(ys)
    return state, sym, mag, first, count


def collect(state, hits, results, check, kept, body, chk_summary, L, R, bits, h, kind, fec, frames_out,
            bodies_out):
    """demod_rx_collect_async. state STATE_DTYPE [S], hits C.HIT_DTYPE [S][mf],
    results RESULT_DTYPE [S], check C.CHECK_DTYPE [S][mf], kept uint32 [S][mf],
    body uint8 [S][mf][max_len], chk_summary C.SUMMARY_DTYPE [S], as stored.
    Returns copies (state, frames, bodies, summary) of the outputs with what
    the call writes laid over frames_out (FRAME_DTYPE [S mf]) and bodies_out
    (uint8 [S mf max_len])."""
    state = state.copy()
    frames, bodies = frames_out.copy(), bodies_out.copy()
    S, mf = hits.shape
    max_len = body.shape[2]
    n, nb, checked, valid = 0, 0, 0, 0
    for s in range(S):
        nw = min(int(results["n_written"][s]), mf)
        nk = min(int(chk_summary["n_kept"][s]), mf)
        base, hold = int(state["base"][s]), int(state["hold"][s])
        reach = hold
        for i in range(nw):
            if check["status"][s, i] == C.OK:
                ln = min(int(check["length"][s, i]), max_len)
                reach = max(reach, (base + int(hits["window"][s, i]) + (L + span(ln, bits, h, kind, fec)) * R) & M64)
        for r in range(nk):
            i = int(kept[s, r])
            if i >= mf:
                continue
            w = (base + int(hits["window"][s, i])) & M64
            if w < hold:
                continue
            ln = min(int(check["length"][s, i]), max_len)
            frames[n] = (s, ln, w, nb, int(hits["errors"][s, i]), 0)
            bodies[nb:nb + ln] = body[s, r, :ln]
            n, nb = n + 1, nb + ln
        fill, tail = int(state["fill"][s]), int(results["tail_window"][s])
        state["hold"][s] = reach
        t = min(tail, fill) if tail >= 0 else fill - (L - 1) * R
        state["keep"][s] = max(0, t - (R - 1))
        cut = int(results["n_hits"][s]) - int(results["n_written"][s])
        state["cut_hits"][s] = (int(state["cut_hits"][s]) + max(cut, 0)) & M64
        checked += min(int(chk_summary["n_checked"][s]), mf)
        valid += min(int(chk_summary["n_valid"][s]), mf)
    summary = np.zeros((), SUMMARY_DTYPE)
    summary["n_frames"], summary["n_bytes"], summary["n_checked"], summary["n_valid"] = n, nb, checked, valid
    return state, frames, bodies, summary


# ---- scan and check of one run of windows ------------------------------------------

def scan_check(sym, P, R, sync, max_errors, N, h, kind, fec, max_frames=None):
    """The scan of (sym, P) as one segment and the check (fec 0) or the mode's
    decode and coded check of its rows. Returns (hits, check, kept, bodies, check
    summary, scan result dict)."""
    sym = np.asarray(sym, np.uint8).reshape(-1)
    P = np.asarray(P, np.float32)
    K, L = P.shape[1], len(sync)
    bits = F.bits_per_symbol(K)
    hits, _, packed, res = FS.frames_segments(sym, P, R, [0], [sym.size], sync, max_errors, N, max_frames)[0]
    group = lambda rows: C.check_group(hits["window"], rows, L, R, Z.span_of(bits, h, kind, fec), None, h, kind)
    if not fec:
        return (hits,) + group(packed) + (res,)
    _, Bd, _ = Z.row_shape(N, bits, h, kind, fec)
    rows = np.zeros((len(hits), Bd), np.uint8)
    if len(hits):
        soft = FEC.soft_bits(P)
        q = np.stack([FEC.row_soft(soft, sym.size, 0, w, L, R, N) for w in hits["window"]])
        written, _ = Z.decode_rows(q, h, kind, fec)
        for i, b in enumerate(written):
            rows[i, :len(b)] = np.frombuffer(b, np.uint8)
    return (hits,) + group(rows) + (res,)


def one_shot(sym, P, R, sync, max_errors, N, h, kind, fec):
    """The kept frames of demod_frames_checked (or demod_frames_coded) on the
    whole recording: [(window, errors, data bytes)]."""
    hits, _, kept, bodies, _, _ = scan_check(sym, P, R, sync, max_errors, N, h, kind, fec)
    return [(int(hits["window"][i]), int(hits["errors"][i]), bodies[r]) for r, i in enumerate(kept)]


class Rx:
    """The receiver of S streams over pieces of detector outputs."""

    def __init__(self, S, K, R, sync, max_errors, N, h, kind, fec, max_frames, ring):
        self.S, self.K, self.R, self.sync = S, K, R, np.asarray(sync, np.uint8)
        self.max_errors, self.N, self.h, self.kind, self.fec = max_errors, N, h, kind, fec
        self.max_frames, self.ring = max_frames, ring
        self.bits = F.bits_per_symbol(K)
        self.state = np.zeros(S, STATE_DTYPE)
        self.sym = [np.zeros(0, np.uint8) for _ in range(S)]
        self.P = [np.zeros((0, K), np.float32) for _ in range(S)]
        self.phases = [[] for _ in range(S)]      # (base + phase) mod R of each scanned push
        self.margins = [[] for _ in range(S)]     # acquire_ref.margin of the same push's metric

    def reset(self, s):
        self.state[s] = 0
        self.sym[s], self.P[s] = np.zeros(0, np.uint8), np.zeros((0, self.K), np.float32)

    def push(self, pieces):
        """pieces: per stream (sym [w], P [w][K]) or None. Returns (frames
        FRAME_DTYPE [n_frames], bodies: a list of bytes, summary)."""
        L, R = len(self.sync), self.R
        frames, bodies, checked, valid, nb = [], [], 0, 0, 0
        for s in range(self.S):
            st = self.state[s]
            new_sym, new_P = pieces[s] if pieces[s] is not None else (np.zeros(0, np.uint8), np.zeros((0, self.K)))
            keep = min(int(st["keep"]), int(st["fill"]))
            ys = np.concatenate([self.sym[s][keep:], np.asarray(new_sym, np.uint8).reshape(-1)])
            yp = np.concatenate([self.P[s][keep:], np.asarray(new_P, np.float32).reshape(-1, self.K)])
            d = max(len(ys) - self.ring, 0)
            self.sym[s], self.P[s] = ys[d:], yp[d:]
            base = int(st["base"]) + keep + d
            st["base"], st["dropped"], st["fill"] = base, int(st["dropped"]) + d, len(ys) - d
            fill = int(st["fill"])
            hits, check, kept, bod, summ, res = scan_check(self.sym[s], self.P[s], R, self.sync, self.max_errors,
                                                           self.N, self.h, self.kind, self.fec, self.max_frames)
            if fill >= R:
                self.phases[s].append((base + res["phase"]) % R)
                self.margins[s].append(acquire_ref.margin(res["metric"]))
            hold = int(st["hold"])
            reach = hold
            for i in np.flatnonzero(check["status"] == C.OK):
                S_i = span(int(check["length"][i]), self.bits, self.h, self.kind, self.fec)
                reach = max(reach, base + int(hits["window"][i]) + (L + S_i) * R)
            for r, i in enumerate(kept):
                w = base + int(hits["window"][i])
                if w >= hold:
                    frames.append((s, len(bod[r]), w, nb, int(hits["errors"][i]), 0))
                    bodies.append(bod[r])
                    nb += len(bod[r])
            st["hold"] = reach
            t = res["tail_window"] if res["tail_window"] >= 0 else fill - (L - 1) * R
            st["keep"] = max(0, t - (R - 1))       # R - 1 more: the word's start on the other phases
            st["cut_hits"] = int(st["cut_hits"]) + res["n_hits"] - res["n_written"]
            checked, valid = checked + int(summ["n_checked"]), valid + int(summ["n_valid"])
        summary = dict(n_frames=len(frames), n_bytes=nb, n_checked=checked, n_valid=valid)
        return np.array(frames, FRAME_DTYPE).reshape(-1), bodies, summary


# ---- recordings: symbol streams with planted frames ---------------------------------

def row_symbols(h, kind, fec, bits, max_len):
    """The smallest N whose rows hold frames of max_len data bytes."""
    return Z.symbols_for(max_len, bits, h, kind, fec)


def frame_symbols(data, word, bits, h, kind, fec):
    """A frame on the air: the word, then the S symbols of its (coded) bytes."""
    raw = Z.encode(data, h, kind, fec) if fec else C.encode(data, h, kind)
    return np.concatenate([np.asarray(word, np.uint8), C.unpack(raw, span(len(data), bits, h, kind, fec), bits)])


def embed(inner, bits, h, lead=8, tail=2):
    """Data bytes of a plain frame that carry the symbols `inner` from payload
    symbol `lead` on (lead * bits a multiple of 8, at or past the header)."""
    assert lead * bits % 8 == 0 and lead * bits >= 8 * h
    b = np.unpackbits(np.asarray(inner, np.uint8)[:, None], axis=1)[:, 8 - bits:].reshape(-1)
    b = np.concatenate([b, np.zeros(-b.size % 8, np.uint8)])
    return bytes([0x5A] * (lead * bits // 8 - h)) + np.packbits(b).tobytes() + bytes([0xC3] * tail)


def stream_symbols(items, K, word, h, kind, fec, rng):
    """items: ints (that many random symbols) and bytes (a frame with that
    data). Returns (symbols, planted: [(symbol index of the word, data)])."""
    bits = F.bits_per_symbol(K)
    out, planted, at = [], [], 0
    for it in items:
        s = rng.integers(0, K, it).astype(np.uint8) if isinstance(it, int) else \
            frame_symbols(it, word, bits, h, kind, fec)
        if not isinstance(it, int):
            planted.append((at, bytes(it)))
        out.append(s)
        at += len(s)
    return np.concatenate(out), planted


def windows_of(symbols, K, R, p0, rng):
    """Detector outputs of a symbol stream whose symbol j decides window p0 +
    j R: there the decided tone's power is 1000 and the others' below 20; the
    R - 1 windows between two symbols hold random symbols with every power
    below 50, so every run of R or more windows has its metric's maximum on
    absolute phase p0 mod R."""
    W = p0 + len(symbols) * R
    sym = rng.integers(0, K, W).astype(np.uint8)
    P = rng.uniform(1.0, 50.0, (W, K)).astype(np.float32)
    on = p0 + np.arange(len(symbols)) * R
    sym[on] = symbols
    P[on] = rng.uniform(1.0, 20.0, (len(symbols), K)).astype(np.float32)
    P[on, symbols] = 1000.0
    return sym, P


def synth_pcm(freqs, symbols, n, seed, sigma=400.0, amplitude=8000.0, fs=48000.0):
    """The symbols as FSK, one per n samples, a random phase per symbol plus
    Gaussian noise (frames_ref.frame_stream's signal)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    ph = rng.uniform(0, 2 * np.pi, len(symbols))
    w = 2 * np.pi * np.asarray(freqs, np.float64)[np.asarray(symbols, np.int64)] / fs
    v = amplitude * np.sin(w[:, None] * t[None, :] + ph[:, None]) + rng.normal(0.0, sigma, (len(symbols), n))
    return np.ascontiguousarray(np.clip(np.round(v), -32768, 32767).astype(np.int16).reshape(-1))
