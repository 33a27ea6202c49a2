"""The link fixture and its ground truth: a transmitter's recording at a chosen
level, cut at any sample, and what a receiver must return from it. The reference
of tests/test_link_cpu.py (tx_ref -> the oracle's double Goertzel -> rx_ref) and
tests/test_gpu_link.py (Transmitter -> Demodulator -> Receiver). numpy only, on
top of tx_ref, rx_ref and frames_check_ref.

The geometry is tx_ref.loopback_case's (n 1024, hop 256, a 16-symbol word, h 1,
CRC-16, frames of 0 .. 3 data bytes with 3 idle symbols behind each, idle (0,
1)); the level, the frame count and the seed are the caller's, and the receiver
runs with max_errors 2. A stream's first `drop` samples are removed, so that a
symbol boundary lies drop samples before a window's start: drop = hop / 2 is
half-way between two window phases.
"""
import numpy as np

import rx_ref as RX
import tx_ref as T

MAX_ERRORS = 2
PACKET = 2880
RAGGED = (1, 7, 997, 2880, 8, 9, T.LOOP_N - 1, T.LOOP_N, T.LOOP_N + 1, 2880, 2880, 2880)   # test_gpu_tx's pulls
R = T.LOOP_N // T.LOOP_HOP
NOISE_SIGMA = 8000
EDGE = {2: 1000, 8: 1400}        # amplitude near the code's edge at NOISE_SIGMA, per K
# the device chain's fixture (tests/test_gpu_link.py; its margins are checked in tests/test_link_cpu.py)
DEV_STREAMS, DEV_FRAMES, DEV_SEED = 8, 6, 0
DEV_DROPS = (0, 100, 120, 128, 129, 136, 200, 255)      # one per stream
DEV_MARGIN = 1e-3                # a hundred times the detectors' 1e-5 magnitude bar
DEV_BAND = T.LOOP_HOP // 16      # |drop - hop / 2| <= DEV_BAND: the phase flips between pushes, the margin crosses 0


def link_case(K, fec, amplitude, sigma, n_frames, seed, lut):
    """Returns (c, datas, N, total): the transmitter's configuration, the frames'
    data, the receiver's row width in symbols and the samples to pull (a
    multiple of PACKET) so that the last frame's row is complete whatever drop
    < n is. lut: oracle.sine_lut()."""
    rng = np.random.default_rng(90000 + 1000 * seed + 10 * K + fec)
    word = rng.integers(0, K, T.LOOP_L).astype(np.uint8)
    datas = [rng.integers(0, 256, int(rng.integers(0, T.LOOP_MAX_LEN + 1))).astype(np.uint8).tobytes()
             for _ in range(n_frames)]
    c = T.make(T.loop_tones(K), T.LOOP_N, lut, word, h=T.LOOP_H, kind=T.LOOP_KIND, fec=fec, max_len=T.LOOP_MAX_LEN,
               gap=3, idle=(0, 1), amplitude=amplitude, sigma=sigma, seed=5000 + 100 * seed + K + fec,
               max_frames=n_frames, stride=PACKET)
    c.C = n_frames * (T.frame_count(c, T.LOOP_MAX_LEN) + c.gap) + 5
    N = RX.row_symbols(T.LOOP_H, T.LOOP_KIND, fec, c.bits, T.LOOP_MAX_LEN)
    symbols = -(-T.LOOP_LEAD // T.LOOP_N) + sum(T.frame_count(c, len(d)) + c.gap for d in datas) + N + 7
    total = -(-symbols * T.LOOP_N // PACKET) * PACKET
    return c, datas, N, total


def recording(c, datas, total, S=1, streams=(0,)):
    """The samples of `streams` out of a transmitter of S: LOOP_LEAD samples of
    idle, every frame in one send, the rest; in PACKET-sample pulls. Returns
    ({stream: samples [total]}, place: the frames' places, the same for each)."""
    tx = T.Tx(c, S)
    counts = [PACKET if s in streams else 0 for s in range(S)]
    out = {s: [] for s in streams}
    place = None
    for at in range(0, total, PACKET):
        if at == T.LOOP_LEAD:
            pl = tx.send([(s, d) for s in streams for d in datas])
            assert pl is not None and (pl["status"] == T.OK).all()
            place = pl[:len(datas)]
        got = tx.pull(counts)
        for s in streams:
            out[s].append(got[s])
    return {s: np.concatenate(out[s]) for s in streams}, place


def sent(place, datas, drop):
    """[(window, data)]: where each frame's word starts in the recording less
    its first `drop` samples, in windows, as a fraction."""
    return [(R * int(p["start"]) - drop / T.LOOP_HOP, bytes(d)) for p, d in zip(place, datas)]


def match(frames, want, R=R):
    """frames: [(window, data)] as returned; want: sent()'s list. Each returned
    frame is paired with a sent frame of the same bytes within R / 2 windows
    that no earlier one took. Returns (delivered: indices into want, ascending;
    false: returned frames near no sent frame of their bytes; double: returned
    frames whose only partners were taken)."""
    used, false, double = set(), [], []
    for w, b in frames:
        near = [i for i, (ws, d) in enumerate(want) if d == bytes(b) and abs(w - ws) <= R / 2]
        free = [i for i in near if i not in used]
        if free:
            used.add(min(free, key=lambda i: abs(w - want[i][0])))
        elif near:
            double.append((w, bytes(b)))
        else:
            false.append((w, bytes(b)))
    return sorted(used), false, double


def packet_sizes(total, drop, scheme):
    """The samples a receiver is pushed per pull of a transmitter that is pulled
    in PACKET-sample packets ("packets") or in RAGGED pieces, the lead apart
    from the rest as tests/test_gpu_tx.py pulls it, when the stream's first
    `drop` samples are removed. They add up to total - drop."""
    sizes, at, k, left = [], 0, 0, drop
    pulls = (PACKET,) if scheme == "packets" else RAGGED
    while at < total:
        m = min(pulls[k % len(pulls)], (T.LOOP_LEAD if at < T.LOOP_LEAD else total) - at)
        k += 1
        cut = min(left, m)
        left -= cut
        sizes.append(m - cut)
        at += m
    assert sum(sizes) == total - drop
    return sizes


def pieces(sym, P, sizes, n=T.LOOP_N, hop=T.LOOP_HOP):
    """The detector outputs (sym [W], P [W][K]) of a recording, cut as a
    receiver that is pushed packets of `sizes` samples sees them: [(sym, P)] per
    push."""
    out, total, seen = [], 0, 0
    for m in sizes:
        total += m
        w = 0 if total < n else (total - n) // hop + 1
        out.append((sym[seen:w], P[seen:w]))
        seen = w
    return out


def run_pushes(rx, cut, s=0):
    """Pushes stream s's pieces `cut` into the reference receiver rx (the other
    streams get nothing). Returns (frames [(window, errors, data)], per push
    (absolute phase or None when nothing was scanned, phase margin or None,
    windows seen so far))."""
    frames, pushes, seen = [], [], 0
    for piece in cut:
        before = len(rx.phases[s])
        fr, bodies, _ = rx.push([piece if t == s else None for t in range(rx.S)])
        seen += len(piece[0])
        scanned = len(rx.phases[s]) > before
        pushes.append((rx.phases[s][-1] if scanned else None, rx.margins[s][-1] if scanned else None, seen))
        frames += [(int(f["window"]), int(f["errors"]), b) for f, b in zip(fr, bodies)]
    return frames, pushes


def completing_push(pushes, window, L, N, R=R):
    """The push in which the row of a hit at `window` is complete: the first
    with more than window + (L + N - 1) R windows seen."""
    for i, (_, _, seen) in enumerate(pushes):
        if seen > window + (L + N - 1) * R:
            return i
    return None
