"""The device chain on tests/link_ref.py's fixture: one Transmitter and one
Receiver of eight streams, each stream cut at its own sample offset (0, 100,
120, 128, 129, 136, 200, 255: on a window, half-way between two window phases
and to either side), the transmitter's own noise on, at the clean level (8000 /
400) and at the edge level of tests/test_link_cpu.py.

Per shape: the transmitter's samples are tx_ref's; the detector's symbols are
the double-precision oracle's on every window of every stream; every push of
the Receiver (records, bytes, every state field of every stream) equals
rx_ref.Rx fed the device detector's own outputs; what comes back was sent, once,
and at the clean level all of it at every offset; and the plain frames equal the
all-double chain's wherever that chain's phase decisions are not near a tie.
"""
import numpy as np
import pytest

import link_ref as LR
import rx_ref as X
import tx_ref as T
from gpu_support import handle_fixture, torch  # noqa: F401

pytestmark = pytest.mark.gpu

N_FFT, HOP, R, L = T.LOOP_N, T.LOOP_HOP, LR.R, T.LOOP_L
S = LR.DEV_STREAMS


@pytest.fixture(scope="module")
def lut(O):
    return O.sine_lut()


# handle(K): one Demodulator (n 1024, hop 256) per K, closed with the module.
handle = handle_fixture(lambda A, K: A.Demodulator(n=N_FFT, hop=HOP, freqs=T.loop_tones(K)))


def tx_cfg(A, c):
    return A.make_tx_cfg(c.sync, c.h, c.kind, c.fec, c.max_len, c.gap, c.idle, c.amplitude, c.sigma, c.seed, c.C,
                         c.max_frames, c.stride)


def pulls_of(total, scheme, group=1):
    """The transmitter's pulls (the lead apart from the rest, as
    link_ref.packet_sizes cuts them), `group` of them to a push."""
    pulls, at, k = [], 0, 0
    sizes = (LR.PACKET,) if scheme == "packets" else LR.RAGGED
    while at < total:
        m = min(sizes[k % len(sizes)], (T.LOOP_LEAD if at < T.LOOP_LEAD else total) - at)
        k += 1
        pulls.append(m)
        at += m
    return [pulls[i:i + group] for i in range(0, len(pulls), group)]


def device_run(A, c, K, fec, datas, N, total, scheme, max_frames=8, ring=None, group=1):
    """Every stream's frames in one send after LOOP_LEAD samples of idle; each
    push takes `group` pulls, stream s less its first DEV_DROPS[s] samples.
    Returns (per stream samples as pulled, places of stream 0's frames, per
    push (records, bodies, the S states), per stream the samples pushed per
    push)."""
    rxcfg = A.make_rx_cfg(c.sync, LR.MAX_ERRORS, N, c.h, c.kind, fec, max_frames, ring or total // HOP + 64)
    pcm, pushes, sizes, left = [[] for _ in range(S)], [], [[] for _ in range(S)], list(LR.DEV_DROPS)
    at, place = 0, None
    with A.Transmitter(S, tx_cfg(A, c), n=N_FFT, hop=HOP, freqs=T.loop_tones(K)) as tx, \
            A.Receiver(S, rxcfg, n=N_FFT, hop=HOP, freqs=T.loop_tones(K)) as rx:
        for pulls in pulls_of(total, scheme, group):
            parts = [[] for _ in range(S)]
            for m in pulls:
                if at == T.LOOP_LEAD:
                    accepted, pl = tx.send([(s, d) for s in range(S) for d in datas])
                    assert accepted == S * len(datas) and (pl["status"] == T.OK).all()
                    place = pl[:len(datas)]
                    assert all(np.array_equal(pl[s * len(datas):(s + 1) * len(datas)], place) for s in range(S))
                out = tx.pull(m)
                at += m
                for s in range(S):
                    pcm[s].append(out[s])
                    cut = min(left[s], m)
                    left[s] -= cut
                    parts[s].append(out[s][cut:])
            packets = [np.concatenate(p) for p in parts]
            for s in range(S):
                sizes[s].append(len(packets[s]))
            fr, bodies, summ = rx.push([p if len(p) else None for p in packets])
            assert summ["n_frames"] == len(fr)
            pushes.append((fr, bodies, [rx.state(s) for s in range(S)]))
    assert at == total and place is not None
    return [np.concatenate(p) for p in pcm], place, pushes, sizes


def detector(d, O, K, pcm):
    """The device detector's (sym, P) of a recording, its symbols held to the
    oracle's double Goertzel on every window. Returns (sym, P, the oracle's P)."""
    W = (len(pcm) - N_FFT) // HOP + 1
    sym, P = d.batch(pcm[:(W - 1) * HOP + N_FFT], mags=True)
    o_sym, o_P = O.goertzel(pcm, T.loop_tones(K), N_FFT, HOP)
    assert len(sym) == len(o_sym) == W
    bad = np.flatnonzero(sym != o_sym)
    assert bad.size == 0, ("detector symbols", bad.size, bad[:8].tolist())
    return sym, P, o_P


def against_reference(c, K, fec, N, max_frames, ring, cuts, pushes):
    """Every push of the device against rx_ref.Rx on the same pieces: records,
    bytes and all state fields of all streams. Returns the reference."""
    ref = X.Rx(S, K, R, c.sync, LR.MAX_ERRORS, N, c.h, c.kind, fec, max_frames, ring)
    for i, (fr, bodies, states) in enumerate(pushes):
        w_fr, w_bodies, _ = ref.push([cuts[s][i] for s in range(S)])
        assert fr.tobytes() == w_fr.tobytes(), ("records", i, fr, w_fr)
        assert bodies == w_bodies, ("bytes", i)
        for s in range(S):
            assert states[s] == {f: int(ref.state[f][s]) for f in X.STATE_DTYPE.names}, ("state", i, s)
    return ref


def frames_of(pushes, s, upto=None):
    return [(int(f["window"]), int(f["errors"]), b) for fr, bodies, _ in pushes[:upto] for f, b in zip(fr, bodies)
            if int(f["stream"]) == s]


def level_of(K, level):
    return (8000, 400) if level == "clean" else (LR.EDGE[K], LR.NOISE_SIGMA)


@pytest.mark.parametrize("scheme", ["packets", "ragged"])
@pytest.mark.parametrize("level", ["clean", "edge"])
@pytest.mark.parametrize("fec", [0, 1])
@pytest.mark.parametrize("K", [2, 8])
def test_link(A, O, torch, handle, lut, K, fec, level, scheme):
    amplitude, sigma = level_of(K, level)
    c, datas, N, total = LR.link_case(K, fec, amplitude, sigma, LR.DEV_FRAMES, LR.DEV_SEED, lut)
    ring = total // HOP + 64
    pcm, place, pushes, sizes = device_run(A, c, K, fec, datas, N, total, scheme)
    # the transmitter's samples
    want, w_place = LR.recording(c, datas, total, S, (0, S - 1))
    assert np.array_equal(place, w_place)
    for s in (0, S - 1):
        assert pcm[s].tobytes() == want[s].tobytes(), ("transmitter samples", s)
    # the detector's symbols; the receiver against the reference on the detector's own outputs
    d = handle(K)
    det = [detector(d, O, K, pcm[s][LR.DEV_DROPS[s]:]) for s in range(S)]
    cuts = [LR.pieces(det[s][0], det[s][1], sizes[s]) for s in range(S)]
    ref = against_reference(c, K, fec, N, 8, ring, cuts, pushes)
    assert (ref.state["dropped"] == 0).all() and (ref.state["cut_hits"] == 0).all()
    # the ground truth
    for s, drop in enumerate(LR.DEV_DROPS):
        got = frames_of(pushes, s)
        delivered, false, double = LR.match([(w, b) for w, _, b in got], LR.sent(place, datas, drop))
        assert not false and not double, ("ground truth", s, false, double)
        if level == "clean":
            assert delivered == list(range(len(datas))) and [b for _, _, b in got] == datas, ("delivery", s, got)
    # plain frames against the all-double chain
    if fec == 0:
        whole = 0
        for s in range(S):
            o_P = det[s][2].astype(np.float32)
            chain = X.Rx(1, K, R, c.sync, LR.MAX_ERRORS, N, c.h, c.kind, 0, 8, ring)
            per_push, marks = [], []
            for piece in LR.pieces(det[s][0], o_P, sizes[s]):
                before = len(chain.margins[0])
                fr, bodies, _ = chain.push([piece])
                per_push.append([(int(f["window"]), int(f["errors"]), b) for f, b in zip(fr, bodies)])
                marks.append(chain.margins[0][-1] if len(chain.margins[0]) > before else 1.0)
            low = [i for i, m in enumerate(marks) if m < LR.DEV_MARGIN]
            upto = low[0] if low else len(marks)       # every push before the first near-tie; all of them if none
            assert frames_of(pushes, s, upto) == [f for p in per_push[:upto] for f in p], ("double chain", s, upto)
            whole += not low
        outside = [dr for dr in LR.DEV_DROPS if abs(dr - HOP // 2) <= LR.DEV_BAND]
        assert whole >= (S - len(outside) if level == "clean" else 2), ("streams compared whole", whole)


@pytest.mark.parametrize("case", ["cut", "smallest ring"])
def test_cut_hits_and_smallest_ring(A, O, torch, handle, lut, case):
    """max_frames 1 with forty pulls to a push, so that two frames complete in
    one push and cut_hits counts; and the ring at the smallest size
    demod_rx_sizes accepts, which the R - 1 windows kept more must still fit.
    Both against the reference on the detector's own outputs, every push."""
    K, fec = 2, 0
    c, datas, N, total = LR.link_case(K, fec, 8000, 400, LR.DEV_FRAMES, LR.DEV_SEED, lut)
    max_frames, ring, group = (1, total // HOP + 64, 40) if case == "cut" else (8, X.min_ring(L, N, R), 1)
    pcm, place, pushes, sizes = device_run(A, c, K, fec, datas, N, total, "packets", max_frames, ring, group)
    d = handle(K)
    det = [detector(d, O, K, pcm[s][LR.DEV_DROPS[s]:]) for s in range(S)]
    cuts = [LR.pieces(det[s][0], det[s][1], sizes[s]) for s in range(S)]
    ref = against_reference(c, K, fec, N, max_frames, ring, cuts, pushes)
    for s, drop in enumerate(LR.DEV_DROPS):
        got = frames_of(pushes, s)
        delivered, false, double = LR.match([(w, b) for w, _, b in got], LR.sent(place, datas, drop))
        assert not false and not double, (s, false, double)
        if case == "cut":
            assert int(ref.state["cut_hits"][s]) == len(datas) - len(delivered) > 0, (s, ref.state[s])
        else:
            assert delivered == list(range(len(datas))) and ref.state["dropped"][s] == 0, (s, got)
            assert max(st[s]["fill"] for _, _, st in pushes) <= ring
    if case == "smallest ring":
        with pytest.raises(A.DemodError):
            A.Receiver(S, A.make_rx_cfg(c.sync, LR.MAX_ERRORS, N, c.h, c.kind, fec, 8, ring - 1), n=N_FFT, hop=HOP,
                       freqs=T.loop_tones(K))
