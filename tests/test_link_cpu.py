"""The live receiver at every symbol-timing offset and in noise, the reference
chain alone: tests/tx_ref.py -> the oracle's double Goertzel (powers cast to
float32) -> tests/rx_ref.py, on tests/link_ref.py's fixture. No device.

Offsets: a stream less its first `drop` samples has its symbol boundaries drop
samples before a window's start; at drop = hop / 2 two window phases see the
same signal and the timing metric of a short run X picks either. A receiver
whose `keep` lies on one push's phase loses the frames whose next push picks
the neighbouring earlier one; with R - 1 windows more kept it returns the
one-shot's frames at every offset.

Noise: what the receiver returns was sent, once; the code pays; and a frame the
one-shot returns is missed by the pushed receiver only where include/demod.h
says it may be.
"""
import numpy as np
import pytest

import link_ref as LR
import rx_ref as X
import tx_ref as T

R, L = LR.R, T.LOOP_L
SHAPES = [(2, 0), (2, 1), (8, 0), (8, 1)]
SCHEMES = ("packets", "ragged")
SWEEP_DROPS = tuple(range(0, T.LOOP_HOP, 8)) + (127, 129, 255)
SWEEP_FRAMES = 6                 # every frame meets the same offset: six show what twelve show
NOISE_SIGMA, NOISE_FRAMES, NOISE_SEEDS, NOISE_DROPS = LR.NOISE_SIGMA, 12, (0, 1, 2, 3), (0, 64, 128, 200)
EDGE = LR.EDGE


@pytest.fixture(scope="module")
def lut(O):
    return O.sine_lut()


def chain(O, c, K, fec, N, pcm):
    """The detector's outputs of a recording and the one-shot's kept frames on
    them: (sym, P float32, [(window, errors, data)], the one-shot's phase)."""
    sym, P = O.goertzel(pcm, T.loop_tones(K), T.LOOP_N, T.LOOP_HOP)
    P = P.astype(np.float32)
    hits, _, kept, bodies, _, res = X.scan_check(sym, P, R, c.sync, LR.MAX_ERRORS, N, c.h, c.kind, fec)
    one = [(int(hits["window"][i]), int(hits["errors"][i]), bodies[r]) for r, i in enumerate(kept)]
    return sym, P, one, int(res["phase"])


def pushed(c, K, fec, N, sym, P, sizes):
    rx = X.Rx(1, K, R, c.sync, LR.MAX_ERRORS, N, c.h, c.kind, fec, 16, len(sym) + 64)
    frames, pushes = LR.run_pushes(rx, LR.pieces(sym, P, sizes))
    st = rx.state[0]
    assert st["dropped"] == 0 and st["cut_hits"] == 0
    assert int(st["base"]) + int(st["fill"]) == len(sym)
    return frames, pushes


@pytest.mark.parametrize("K,fec", SHAPES)
def test_every_offset_at_the_clean_level(O, lut, K, fec):
    """A 8000, sigma 400, drops 0, 8, .., 248 and 127, 129, 255. The one-shot
    returns every sent frame (a condition of the fixture); the pushed receiver
    returns the same frames once each, in order, with the same bytes, in
    2880-sample packets and in ragged ones: at the one-shot's window where the
    completing push chose the one-shot's absolute phase, within R - 1 windows
    of it otherwise."""
    c, datas, N, total = LR.link_case(K, fec, 8000, 400, SWEEP_FRAMES, 0, lut)
    rec, place = LR.recording(c, datas, total)
    failed = []
    for drop in SWEEP_DROPS:
        sym, P, one, phase = chain(O, c, K, fec, N, rec[0][drop:])
        want = LR.sent(place, datas, drop)
        delivered, false, double = LR.match([(w, b) for w, _, b in one], want)
        assert delivered == list(range(len(datas))) and not false and not double, ("one-shot", drop)
        assert len(one) == len(datas)
        for scheme in SCHEMES:
            got, pushes = pushed(c, K, fec, N, sym, P, LR.packet_sizes(total, drop, scheme))
            ok = [b for _, _, b in got] == [b for _, _, b in one]
            for (w, _, _), (w1, _, _) in zip(got, one) if ok else ():
                # windows are absolute: w mod R is the absolute phase of the push that returned the frame
                ok = ok and (w == w1 if w % R == phase else abs(w - w1) <= R - 1)
            if not ok:
                failed.append((drop, scheme, [(w, b) for w, _, b in got]))
    assert not failed, (len(failed), sorted({d for d, _, _ in failed}), failed[0])


def noise_level(O, lut, K, fec, amplitude):
    """One level's streams (NOISE_SEEDS x NOISE_DROPS x SCHEMES): every check
    that holds per stream, and the level's counts (one-shot delivered, pushed
    delivered, exempted)."""
    n_one, n_pushed, n_exempt = 0, 0, 0
    for seed in NOISE_SEEDS:
        c, datas, N, total = LR.link_case(K, fec, amplitude, NOISE_SIGMA, NOISE_FRAMES, seed, lut)
        rec, place = LR.recording(c, datas, total)
        for drop in NOISE_DROPS:
            sym, P, one, phase = chain(O, c, K, fec, N, rec[0][drop:])
            want = LR.sent(place, datas, drop)
            d_one, false, double = LR.match([(w, b) for w, _, b in one], want)
            assert not false and not double, ("one-shot", seed, drop, false, double)
            window_of = {}
            for w, _, b in one:
                for i in LR.match([(w, b)], want)[0]:
                    window_of.setdefault(i, w)
            for scheme in SCHEMES:
                got, pushes = pushed(c, K, fec, N, sym, P, LR.packet_sizes(total, drop, scheme))
                d_got, false, double = LR.match([(w, b) for w, _, b in got], want)
                assert not false, ("returned, never sent", seed, drop, scheme, false)
                assert not double, ("returned twice", seed, drop, scheme, double)
                assert [w for w, _, _ in got] == sorted(w for w, _, _ in got)
                for i in set(d_one) - set(d_got):
                    w = window_of[i]
                    fits = [j for j, (_, _, seen) in enumerate(pushes) if seen > w + (L - 1) * R][0]
                    done = LR.completing_push(pushes, w, L, N)
                    other = [pushes[j][0] for j in range(fits, done + 1) if pushes[j][0] != phase]
                    assert other, ("missed under the one-shot's phase throughout", seed, drop, scheme, w)
                    n_exempt += 1
                n_one, n_pushed = n_one + len(d_one), n_pushed + len(d_got)
    return n_one, n_pushed, n_exempt


@pytest.mark.parametrize("K", [2, 8])
def test_noise(O, lut, K):
    """sigma 8000 at amplitudes 8000, 3000 and EDGE[K]; four seeds, drops 0, 64,
    128, 200, twelve frames a stream, both packet schemes. Nothing returned was
    not sent, nothing is returned twice. A frame the one-shot returns and the
    pushed receiver misses has a push, from the one in which its word first
    fits to the one in which its row is complete, whose absolute phase is not
    the one-shot's (include/demod.h "receiver"); over a level's streams those
    are at most half of what the one-shot returns. The code pays: coded
    one-shot delivery is at least the plain one's at every level and strictly
    more at the edge.

    The narrower claim, that the completing push alone differs, does not hold
    in the reference: at K 2 coded, 1000 / 8000, 17 of the 47 missed frames (of
    338) complete under the one-shot's phase; an earlier push on another phase
    found no word there (more than max_errors errors) and let the start go."""
    for amplitude in (8000, 3000, EDGE[K]):
        one = {}
        for fec in (0, 1):
            n_one, n_pushed, n_exempt = noise_level(O, lut, K, fec, amplitude)
            print(f"K {K} fec {fec} A {amplitude}: one-shot {n_one} pushed {n_pushed} exempt {n_exempt}")
            assert 2 * n_exempt <= n_one, (amplitude, fec, n_one, n_exempt)
            one[fec] = n_one
        assert one[1] >= one[0], (amplitude, one)
        if amplitude == EDGE[K]:
            assert one[1] > one[0], (amplitude, one)
        else:
            full = len(NOISE_SEEDS) * len(NOISE_DROPS) * len(SCHEMES) * NOISE_FRAMES
            assert one[1] == full, "above the edge the coded one-shot returns every frame"


def test_match_tells_false_and_double():
    """The ground truth's own cases: a frame half a symbol off is delivered, one
    a symbol off or with other bytes is false, a second copy is double."""
    want = [(100.5, b"ab"), (300.0, b""), (500.25, b"ab")]
    assert LR.match([(101, b"ab"), (300, b""), (499, b"ab")], want) == ([0, 1, 2], [], [])
    assert LR.match([(104, b"ab")], want) == ([], [(104, b"ab")], [])
    assert LR.match([(300, b"x")], want) == ([], [(300, b"x")], [])
    assert LR.match([(100, b"ab"), (102, b"ab")], want) == ([0], [], [(102, b"ab")])
    assert LR.match([(302, b""), (298, b"")], want) == ([1], [], [(298, b"")])


def test_packet_sizes_and_pieces():
    """The cut: sizes add up to the recording, the pieces to all its windows,
    and a window belongs to the push that brings its last sample."""
    total, drop = 10 * LR.PACKET, 129
    for scheme in SCHEMES:
        sizes = LR.packet_sizes(total, drop, scheme)
        assert sum(sizes) == total - drop and min(sizes) >= 0
        W = (total - drop - T.LOOP_N) // T.LOOP_HOP + 1
        sym, P = np.arange(W) % 251, np.arange(2 * W).reshape(W, 2)
        cut = LR.pieces(sym.astype(np.uint8), P, sizes)
        assert np.array_equal(np.concatenate([s for s, _ in cut]), sym)
        assert np.array_equal(np.concatenate([p for _, p in cut]), P)
        seen, samples = 0, 0
        for (s, _), m in zip(cut, sizes):
            samples += m
            seen += len(s)
            assert seen == max(0, (samples - T.LOOP_N) // T.LOOP_HOP + 1)
    assert LR.packet_sizes(total, 0, "packets") == [LR.PACKET] * 10


@pytest.mark.parametrize("K", [2, 8])
def test_device_fixture_margins(O, lut, K):
    """tests/test_gpu_link.py holds the device's plain frames to this chain's on
    every stream whose pushes all decide their phase by a margin of DEV_MARGIN
    or more, and on the others up to their first push below it. Which streams
    those are, with both packet schemes: at the clean level every stream but
    the four whose drop lies within DEV_BAND of hop / 2 (120, 128, 129, 136:
    there the two phases tie and the choice flips from push to push, so the
    margin passes through 0; lowest margins measured 1e-7 .. 5e-4); at the edge
    level the noise decides, and at least two of the eight qualify (measured:
    3 to 6).

    A cap of two streams outside cannot be met with these drops: four of them
    lie in the band that loses frames on the parent commit because the phase
    flips."""
    for amplitude, sigma in ((8000, 400), (EDGE[K], NOISE_SIGMA)):
        c, datas, N, total = LR.link_case(K, 0, amplitude, sigma, LR.DEV_FRAMES, LR.DEV_SEED, lut)
        rec, _ = LR.recording(c, datas, total, LR.DEV_STREAMS, range(LR.DEV_STREAMS))
        for scheme in SCHEMES:
            low = []
            for s, drop in enumerate(LR.DEV_DROPS):
                sym, P, _, _ = chain(O, c, K, 0, N, rec[s][drop:])
                _, pushes = pushed(c, K, 0, N, sym, P, LR.packet_sizes(total, drop, scheme))
                low.append(min(m for _, m, _ in pushes if m is not None))
            print(f"K {K} A {amplitude} {scheme}: lowest margins", ["%.2e" % m for m in low])
            outside = [d for d, m in zip(LR.DEV_DROPS, low) if m < LR.DEV_MARGIN]
            if sigma == 400:
                assert outside == [d for d in LR.DEV_DROPS if abs(d - T.LOOP_HOP // 2) <= LR.DEV_BAND], low
            else:
                assert len(outside) <= LR.DEV_STREAMS - 2, low
