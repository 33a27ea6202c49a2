"""The transmitter on the GPU (frames_tx.hip, demod_tx.cpp) against
tests/tx_ref.py.

Stage level: demod_tx_encode_async and demod_tx_modulate_async on hand-made
states, rings and records. Every output is poisoned and compared WHOLE with the
reference laid over the same poison, between guard bands (tests/guards.py): one
comparison says that what must be written is written, byte for byte, and that
nothing else is.

Handle level: frames -> demod_tx_send -> demod_tx_pull -> demod_rx_push returns
every accepted frame once, with its bytes, at R start, in all four formats and
whatever the packet sizes; the handle's samples on the device go through the
detector and the segmented frame scan without leaving it.
"""
import numpy as np
import pytest

import frames_check_ref as C
import guards as G
import rx_ref as X
import tx_ref as T
from gpu_support import handle_fixture, same, torch  # noqa: F401

pytestmark = pytest.mark.gpu

LEAD = 4096                      # guard bytes per side (a multiple of 16: aligned outputs stay aligned)
POISONS = (0xFF, 0x5A)


@pytest.fixture(scope="module")
def lut(O):
    return O.sine_lut()


def tones(K):
    return T.loop_tones(K)


# handle(K, n): one Demodulator (hop n / 4) per (K, n), closed with the module.
handle = handle_fixture(lambda A, K, n: A.Demodulator(n=n, hop=n // 4, freqs=tones(K)))


class Outs:
    """Guarded, poisoned device outputs of one call."""

    def __init__(self, torch, poison):
        self.torch, self.poison, self.checks = torch, poison, []

    def u8(self, nbytes, init=None):
        t, chk = G.guarded(self.torch, max(nbytes, 16), self.torch.uint8, LEAD, LEAD, self.poison)
        self.checks.append(chk)
        t = t[:nbytes]
        if init is not None:
            t.copy_(self.torch.from_numpy(np.ascontiguousarray(init).view(np.uint8).reshape(-1)))
        return t

    def guards_intact(self):
        self.torch.cuda.synchronize()
        for chk in self.checks:
            chk(written=False)


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def tx_cfg(A, c):
    return A.make_tx_cfg(c.sync, c.h, c.kind, c.fec, c.max_len, c.gap, c.idle, c.amplitude, c.sigma, c.seed, c.C,
                         c.max_frames, c.stride)


def dev_u32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def poisoned(shape, dtype, poison):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.full(n, poison, np.uint8).view(dtype).reshape(shape)


# ---- encode ----------------------------------------------------------------------------

def random_state(c, S, rng):
    """States that meet every clamp: tail below head, tail above head + C, an
    offset at or above n, beside ordinary ones with any fill."""
    st = np.zeros(S, T.STATE_DTYPE)
    st["head"] = rng.integers(0, 2 ** 40, S)
    st["offset"] = rng.integers(0, c.n, S)
    st["offset"][::3] = 0
    st["phase"] = rng.integers(0, 2 ** 32, S)
    st["accepted"], st["refused"] = rng.integers(0, 2 ** 40, (2, S))
    used = rng.integers(0, c.C + 1, S)
    used[::2] = rng.integers(0, 8, (S + 1) // 2)
    st["tail"] = st["head"] + np.maximum(used, st["offset"] > 0).astype(np.uint64)
    for s in range(S):
        head = int(st["head"][s])
        if s % 7 == 3:
            st["tail"][s] = head - min(5, head)                            # below head
        if s % 7 == 5:
            st["tail"][s] = head + c.C + 9                                 # above head + C
        if s % 5 == 2:
            st["offset"][s] = c.n + 3                                      # clamped to n - 1
    return st


def encode_case(c, S, seed, long_run):
    """Records, counts and bytes: counts 0 .. max_frames and one stored above;
    lengths from {0, 1, 63, 64, 65, max_len} and random ones; a frame above
    max_len between two good ones; body offsets at and past n_bytes; a stream
    whose ring has room for exactly half its frames (stream 0, when max_frames
    >= 4); with long_run stream 1 sends max_frames frames of length 0 and 1 into
    an empty ring: more than two wave steps of the plan when max_frames is 130."""
    rng = np.random.default_rng(seed)
    mf = c.max_frames
    state = random_state(c, S, rng)
    lens_pool = [ln for ln in (0, 1, 63, 64, 65, c.max_len) if ln <= c.max_len]
    records = np.zeros((S, mf), T.RECORD_DTYPE)
    records["length"] = rng.integers(0, 2 ** 32, (S, mf))          # rows at and past the count: never read
    records["body"] = rng.integers(0, 2 ** 32, (S, mf))
    count = np.zeros(S, np.uint32)
    data = rng.integers(0, 256, 4 * c.max_len + 40).astype(np.uint8)
    for s in range(S):
        cnt = 0 if s % 4 == 3 else int(rng.integers(1, min(mf, 6) + 1))
        for i in range(cnt):
            ln = lens_pool[int(rng.integers(0, len(lens_pool)))] if rng.integers(0, 2) else \
                int(rng.integers(0, c.max_len + 1))
            records[s, i] = (ln, int(rng.integers(0, data.size - ln + 1)))
        if s % 6 == 2 and cnt >= 3:
            records["length"][s, 1] = c.max_len + 1 + (s % 3) * 2 ** 20     # refused between two good ones
        if s % 5 == 1 and cnt:
            records["body"][s, cnt - 1] = data.size + (5 if s % 2 else 0)   # at and past n_bytes: clamped
        count[s] = cnt if s % 9 != 4 or cnt < mf else mf + 3               # stored above max_frames
    if mf >= 4:
        k = mf // 2 if not long_run else 3
        a = T.frame_count(c, 1) + c.gap
        if k * a <= c.C:
            state["offset"][0] = 0
            state["tail"][0] = int(state["head"][0]) + c.C - k * a         # room for exactly k of them
            records[0, :min(mf, k + 2)] = (1, 7)
            count[0] = min(mf, k + 2)
    if long_run and S > 1:
        state["tail"][1], state["offset"][1] = state["head"][1], 0
        records["length"][1, :] = np.arange(mf) % 2
        records["body"][1, :] = np.arange(mf)
        count[1] = mf
    return state, records, count, data


def run_encode(A, torch, d, c, S, state, ring, records, count, data, poison, what):
    x = tx_cfg(A, c)
    o = Outs(torch, poison)
    d_state = o.u8(S * 40, init=state)
    d_ring = o.u8(S * c.C, init=ring)
    d_place = o.u8(S * c.max_frames * 16)
    d_rec = torch.from_numpy(records.view(np.uint8).reshape(-1).copy()).cuda()
    d_bytes = torch.from_numpy(data.copy()).cuda() if data.size else None
    d.tx_encode_async(x, d_state, d_ring, d_rec, dev_u32(torch, count), d_bytes, data.size, S, d_place)
    o.guards_intact()
    place0 = poisoned((S, c.max_frames), T.PLACE_DTYPE, poison)
    w_state, w_ring, w_place = T.send(c, state, ring, records, count, data, place0)
    same(host(d_place, np.uint8), w_place.view(np.uint8), (what, "place"))
    same(host(d_state, np.uint8), w_state.view(np.uint8), (what, "state"))
    same(host(d_ring, np.uint8), w_ring, (what, "ring"))
    return w_state, w_place


ENCODE_CASES = [  # S, max_frames, K, h, kind, fec, gap, long_run
    (1, 1, 2, 1, C.CRC16, 0, 0, False),
    (3, 5, 4, 2, C.CRC32, 1, 3, False),
    (64, 130, 16, 1, C.CRC16, 0, 3, True),
    (65, 5, 8, 2, C.CRC16, 1, 0, False),
    (65, 130, 2, 2, C.CRC32, 1, 3, True),
    (1025, 1, 8, 1, C.CRC32, 0, 3, False),
    (1025, 5, 2, 2, C.CRC16, 0, 0, False),
    (1025, 130, 4, 1, C.CRC16, 0, 3, True),      # 15 waves a group: more frames than waves
]


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("case", ENCODE_CASES)
def test_encode(A, torch, handle, lut, case, poison):
    S, mf, K, h, kind, fec, gap, long_run = case
    n = 256
    word = (np.arange(16) * 7 // 3) % K
    c = T.make(tones(K), n, lut, word, h=h, kind=kind, fec=fec, max_len=65, gap=gap, idle=(1, 0, 1, 1, 0),
               max_frames=mf, stride=2880)
    short = T.frame_count(c, 1) + gap
    c.C = max(3 * (T.frame_count(c, 65) + gap) + 5, (mf + 10) * short if long_run else 0)
    state, records, count, data = encode_case(c, S, 31 * S + mf + K, long_run)
    ring = np.full((S, c.C), poison, np.uint8)
    w_state, w_place = run_encode(A, torch, handle(K, n), c, S, state, ring, records, count, data, poison, case)
    seen = {int(v) for s in range(S) for v in w_place["status"][s, :min(int(count[s]), mf)]}
    if S >= 64 and mf >= 5:
        assert seen == {T.OK, T.BAD_LENGTH, T.NO_ROOM}, seen         # the fixture meets every status
    if long_run:
        assert (w_place["status"][1] == T.OK).all() and mf == 130    # three wave steps, all accepted


@pytest.mark.parametrize("fec", [0, 1])
@pytest.mark.parametrize("kind", [C.CRC16, C.CRC32])
@pytest.mark.parametrize("K", [2, 4, 8, 16])
def test_encode_formats(A, torch, handle, lut, K, kind, fec):
    """All four formats at every K: lengths 0, 1, 63, 64, 65 and max_len in one
    stream, in an order that wraps the ring; gap 0 (plain) and 3 (coded)."""
    n, S, lens = 256, 2, (64, 0, 65, 1, 63, 80)
    c = T.make(tones(K), n, lut, (np.arange(24) * 5) % K, h=2, kind=kind, fec=fec, max_len=80, gap=3 * fec,
               idle=(0, K - 1), max_frames=8, stride=2880)
    c.C = sum(T.frame_count(c, ln) + c.gap for ln in lens) + 2
    rng = np.random.default_rng(K + kind + fec)
    data = rng.integers(0, 256, 400).astype(np.uint8)
    state = np.zeros(S, T.STATE_DTYPE)
    state["head"] = state["tail"] = [3 * c.C + c.C - 40, 2 ** 33 + 17]        # both runs wrap the ring
    records = np.zeros((S, 8), T.RECORD_DTYPE)
    for s in range(S):
        for i, ln in enumerate(lens if s == 0 else lens[::-1]):
            records[s, i] = (ln, 13 * i + s)
    count = np.array([6, 6], np.uint32)
    for poison in POISONS:
        ring = np.full((S, c.C), poison, np.uint8)
        _, place = run_encode(A, torch, handle(K, n), c, S, state, ring, records, count, data, poison, (K, kind, fec))
        assert (place["status"] == T.OK)[:, :6].all()


@pytest.mark.parametrize("K,kind,fec", [(2, C.CRC16, 0), (16, C.CRC32, 1), (8, C.CRC16, 1)])
def test_encode_longest_frame(A, torch, handle, lut, K, kind, fec):
    """One frame of DEMOD_MAX_FRAME_PAYLOAD bytes: every lane's chunk of the CRC
    is 65 bytes, and the coded frame is 65644 bits."""
    n, S = 256, 1
    c = T.make(tones(K), n, lut, [1, 0, 1], h=2, kind=kind, fec=fec, max_len=4096, gap=1, idle=(1,), max_frames=2,
               stride=2880)
    rng = np.random.default_rng(K)
    data = rng.integers(0, 256, 4096 + 9).astype(np.uint8)
    state = np.zeros(S, T.STATE_DTYPE)
    state["head"] = state["tail"] = c.C - 100
    records = np.array([[(4096, 9), (4096, 0)]], T.RECORD_DTYPE)
    ring = np.full((S, c.C), 0xFF, np.uint8)
    _, place = run_encode(A, torch, handle(K, n), c, S, state, ring, records, np.array([2], np.uint32), data, 0xFF,
                          (K, kind, fec))
    assert place["status"].tolist() == [[T.OK, T.NO_ROOM]]


# ---- modulate --------------------------------------------------------------------------

def run_modulate(A, torch, d, c, S, state, ring, count, poison, what):
    x = tx_cfg(A, c)
    o = Outs(torch, poison)
    d_state = o.u8(S * 40, init=state)
    d_ring = o.u8(S * c.C, init=ring)
    d_pcm = o.u8(S * c.stride * 2).view(torch.int16)
    d_work = torch.empty(A.tx_modulate_workspace_size(d.cfg, x, S), dtype=torch.uint8, device="cuda")
    d_work.fill_(poison)
    d.tx_modulate_async(x, d_state, d_ring, dev_u32(torch, count), S, d_pcm, d_work)
    o.guards_intact()
    pcm0 = poisoned((S, c.stride), np.int16, poison)
    w_state, w_ring, w_pcm = T.modulate(c, state, ring, count, pcm0)
    same(host(d_pcm, np.int16), w_pcm, (what, "pcm"))
    same(host(d_state, np.uint8), w_state.view(np.uint8), (what, "state"))
    same(host(d_ring, np.uint8), w_ring, (what, "ring"))
    return w_state, w_ring, w_pcm


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("S,K,sigma,amplitude", [(1, 2, 0, 8000), (3, 8, 400, 8000), (65, 4, 400, 8000),
                                                 (300, 16, 20000, 32767), (65, 2, 0, 32767)])
def test_modulate(A, torch, handle, lut, S, K, sigma, amplitude, poison):
    """m in {0, 1, 7, 8, 9, n - 1, n, n + 1, 2880, 200 symbols and more} mixed
    across the streams of one call, stored counts above the stride, offsets
    mid-symbol, queues that run dry inside the pull, rings that wrap inside it,
    ring bytes at and above K, clipping (amplitude 32767 with sigma 20000). The
    phase launch runs ceil(symbols / 256) waves a stream, 16 at most: 1 wave
    (S = 300, 200 symbols), 4 and 5 either side of 1024 symbols (S = 3, 65, 65),
    and 16 waves whose carry crosses three steps of 4096 symbols (S = 1)."""
    n = 256
    long = {1: 8300, 3: 1021, 65: 1025}.get(S, 200)
    c = T.make(tones(K), n, lut, [0, 1], max_len=4, idle=(1, 0, 0, 1, 1) if K == 2 else (K - 1, 0, 2), amplitude=amplitude,
               sigma=sigma, seed=99 + S, max_frames=1, stride=long * n + 8, ring=97)
    rng = np.random.default_rng(1000 * S + K + sigma)
    state = random_state(c, S, rng)
    ring = rng.integers(0, 256, (S, c.C)).astype(np.uint8)        # & 15 gives tones at and above K: silent
    ms = [0, 1, 7, 8, 9, n - 1, n, n + 1, 2880, long * n, c.stride, c.stride + 1000, 2 ** 32 - 1]
    count = np.array([ms[(s + S) % len(ms)] for s in range(S)], np.uint32)
    if S == 1:
        count[0] = long * n + 3                                   # the carry crosses three wave steps
    if S >= 3:                                                    # a full ring, read across its wrap
        state["offset"][1], state["head"][1] = 5, 2 ** 35 + c.C - 3
        state["tail"][1] = 2 ** 35 + c.C - 3 + c.C
        count[1] = 40 * n
    w_state, _, w_pcm = run_modulate(A, torch, handle(K, n), c, S, state, ring, count, poison, (S, K))
    if sigma == 20000:
        assert (w_pcm == 32767).any() and (w_pcm == -32768).any()


@pytest.mark.parametrize("K,fec", [(2, 0), (8, 1)])
def test_ragged_pulls_equal_one(A, torch, handle, lut, K, fec):
    """Encode and modulate chained on the device, a send between the pulls: a
    stream pulled in ragged pieces is, byte for byte, the stream pulled whole,
    and both are the reference's."""
    n, S = 256, 3
    c = T.make(tones(K), n, lut, np.arange(8) % K, h=1, kind=C.CRC16, fec=fec, max_len=4, gap=2, idle=(1, 0, 0),
               amplitude=9000, sigma=300, seed=5, max_frames=2, stride=2880)
    c.C = 2 * (T.frame_count(c, 4) + 2) + 3
    x, d = tx_cfg(A, c), handle(K, n)
    frames = [(1, b"\x01\x02\x03\x04"), (0, b""), (1, b"z"), (2, b"abc")]
    first = 2 * n + 17
    total = first + (c.C + 6) * n + 5
    ref = T.Tx(c, S)
    want = [ref.pull(first)]
    assert (ref.send(frames)["status"] == T.OK).all()
    left = total - first
    while left:
        want.append(ref.pull(min(left, c.stride)))
        left -= min(left, c.stride)
    want = [np.concatenate([w[s] for w in want]) for s in range(S)]
    records = np.zeros((S, 2), T.RECORD_DTYPE)
    records[1, 0], records[0, 0], records[1, 1], records[2, 0] = (4, 0), (0, 4), (1, 4), (3, 5)
    data = np.frombuffer(b"\x01\x02\x03\x04zabc", np.uint8)
    d_rec = torch.from_numpy(records.view(np.uint8).reshape(-1).copy()).cuda()
    d_bytes = torch.from_numpy(data.copy()).cuda()
    d_fcount = dev_u32(torch, [1, 2, 1])
    for pieces in ([2880], [1, 7, 8, 9, n - 1, n, n + 1, 2880, 100]):
        d_state = torch.zeros(S * 40, dtype=torch.uint8, device="cuda")
        d_ring = torch.zeros(S * c.C, dtype=torch.uint8, device="cuda")
        d_place = torch.zeros(S * 2 * 16, dtype=torch.uint8, device="cuda")
        d_pcm = torch.zeros(S * c.stride, dtype=torch.int16, device="cuda")
        d_work = torch.empty(A.tx_modulate_workspace_size(d.cfg, x, S), dtype=torch.uint8, device="cuda")
        got, at, k = [[] for _ in range(S)], 0, 0
        while at < total:
            if at == first:
                d.tx_encode_async(x, d_state, d_ring, d_rec, d_fcount, d_bytes, data.size, S, d_place)
            m = min(pieces[k % len(pieces)], (first if at < first else total) - at)
            k += 1
            d.tx_modulate_async(x, d_state, d_ring, dev_u32(torch, [m] * S), S, d_pcm, d_work)
            out = d_pcm.cpu().numpy().reshape(S, c.stride)
            for s in range(S):
                got[s].append(out[s, :m].copy())
            at += m
        for s in range(S):
            same(np.concatenate(got[s]), want[s], (pieces[0], s))
        same(host(d_state, np.uint8), ref.state.view(np.uint8), (pieces[0], "state"))


def test_capture_and_replay(A, torch, handle, lut):
    """Encode + modulate captured once on a side stream and replayed after the
    records, bytes and counts were rewritten in place: each replay's outputs are
    the eager run's and the reference's for that content."""
    K, n, S, mf = 4, 256, 5, 3
    c = T.make(tones(K), n, lut, [3, 1, 0, 2], h=1, kind=C.CRC32, fec=1, max_len=6, gap=1, idle=(2, 1), sigma=200,
               seed=3, max_frames=mf, stride=2880)
    c.C = 3 * (T.frame_count(c, 6) + 1)
    x, d = tx_cfg(A, c), handle(K, n)
    contents = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        records = np.zeros((S, mf), T.RECORD_DTYPE)
        records["length"] = rng.integers(0, 8, (S, mf))
        records["body"] = rng.integers(0, 30, (S, mf))
        contents.append((records, rng.integers(0, mf + 2, S).astype(np.uint32),
                         rng.integers(0, 256, 32).astype(np.uint8), rng.integers(0, 2881, S).astype(np.uint32)))
    d_state = torch.zeros(S * 40, dtype=torch.uint8, device="cuda")
    d_ring = torch.zeros(S * c.C, dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros(S * mf * 8, dtype=torch.uint8, device="cuda")
    d_fcount = torch.zeros(S, dtype=torch.int32, device="cuda")
    d_bytes = torch.zeros(32, dtype=torch.uint8, device="cuda")
    d_count = torch.zeros(S, dtype=torch.int32, device="cuda")
    d_place = torch.zeros(S * mf * 16, dtype=torch.uint8, device="cuda")
    d_pcm = torch.zeros(S * c.stride, dtype=torch.int16, device="cuda")
    d_work = torch.empty(A.tx_modulate_workspace_size(d.cfg, x, S), dtype=torch.uint8, device="cuda")

    def load(content):
        records, fcount, data, count = content
        d_rec.copy_(torch.from_numpy(records.view(np.uint8).reshape(-1).copy()))
        d_fcount.copy_(torch.from_numpy(fcount.view(np.int32)))
        d_bytes.copy_(torch.from_numpy(data))
        d_count.copy_(torch.from_numpy(count.view(np.int32)))
        d_place.fill_(0x5A)
        d_pcm.fill_(0x5A5A)

    def step(stream):
        d.tx_encode_async(x, d_state, d_ring, d_rec, d_fcount, d_bytes, 32, S, d_place, stream=stream)
        d.tx_modulate_async(x, d_state, d_ring, d_count, S, d_pcm, d_work, stream=stream)

    def reference(state, ring, content):
        records, fcount, data, count = content
        state, ring, place = T.send(c, state, ring, records, fcount, data, poisoned((S, mf), T.PLACE_DTYPE, 0x5A))
        state, ring, pcm = T.modulate(c, state, ring, count, poisoned((S, c.stride), np.int16, 0x5A))
        return state, ring, place, pcm

    r_state, r_ring = np.zeros(S, T.STATE_DTYPE), np.zeros((S, c.C), np.uint8)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        load(contents[0])
        step(side.cuda_stream)                      # an eager call of the shape first (the sine table goes up)
        side.synchronize()
    r_state, r_ring, place, pcm = reference(r_state, r_ring, contents[0])
    same(host(d_pcm, np.int16), pcm, "eager pcm")
    same(host(d_place, np.uint8), place.view(np.uint8), "eager place")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step(torch.cuda.current_stream().cuda_stream)
    # the capture itself runs nothing: the state is still the eager call's
    for rep, content in enumerate((contents[1], contents[0], contents[1])):
        load(content)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        r_state, r_ring, place, pcm = reference(r_state, r_ring, content)
        same(host(d_pcm, np.int16), pcm, (rep, "pcm"))
        same(host(d_place, np.uint8), place.view(np.uint8), (rep, "place"))
        same(host(d_state, np.uint8), r_state.view(np.uint8), (rep, "state"))
        same(host(d_ring, np.uint8), r_ring, (rep, "ring"))


def test_stage_refusals(A, torch, handle, lut):
    K, n, S = 2, 256, 2
    c = T.make(tones(K), n, lut, [0, 1], max_len=4, max_frames=2, stride=2880)
    x, d = tx_cfg(A, c), handle(K, n)
    u8 = lambda nb: torch.zeros(nb, dtype=torch.uint8, device="cuda")
    state, ring, rec, place = u8(S * 40 + 8), u8(S * c.C), u8(S * 2 * 8 + 8), u8(S * 2 * 16 + 8)
    cnt = torch.zeros(S + 1, dtype=torch.int32, device="cuda")
    pcm = torch.zeros(S * c.stride + 8, dtype=torch.int16, device="cuda")
    work = u8(A.tx_modulate_workspace_size(d.cfg, x, S) + 8)
    lib, ref = A.load_library(), __import__("ctypes").byref
    p = lambda t, off=0: t.data_ptr() + off
    enc = lambda *a: lib.demod_tx_encode_async(*a)
    ok = (d._h, ref(x), p(state), p(ring), p(rec), p(cnt), None, 0, S, p(place), None)
    assert enc(*ok) == A.DEMOD_OK
    for i in (0, 2, 3, 4, 5, 9):                                             # a NULL handle or pointer
        assert enc(*[None if j == i else v for j, v in enumerate(ok)]) == A.DEMOD_BAD_ARG, i
    assert enc(d._h, ref(x), p(state, 4), p(ring), p(rec), p(cnt), None, 0, S, p(place), None) == A.DEMOD_BAD_ARG
    assert enc(d._h, ref(x), p(state), p(ring), p(rec, 2), p(cnt), None, 0, S, p(place), None) == A.DEMOD_BAD_ARG
    assert enc(d._h, ref(x), p(state), p(ring), p(rec), p(cnt), None, 0, S, p(place, 4), None) == A.DEMOD_BAD_ARG
    assert enc(d._h, ref(x), p(state), p(ring), p(rec), p(cnt), None, 5, S, p(place), None) == A.DEMOD_BAD_ARG
    assert enc(d._h, ref(x), p(state), p(ring), p(rec), p(cnt), None, 0, 0, p(place), None) == A.DEMOD_BAD_ARG
    mod = lambda *a: lib.demod_tx_modulate_async(*a)
    ok = (d._h, ref(x), p(state), p(ring), p(cnt), S, p(pcm), p(work), work.numel(), None)
    assert mod(*ok) == A.DEMOD_OK
    for i in (0, 2, 3, 4, 6, 7):
        assert mod(*[None if j == i else v for j, v in enumerate(ok)]) == A.DEMOD_BAD_ARG, i
    assert mod(d._h, ref(x), p(state), p(ring), p(cnt), S, p(pcm, 8), p(work), work.numel(), None) == A.DEMOD_BAD_ARG
    assert mod(d._h, ref(x), p(state), p(ring), p(cnt), S, p(pcm), p(work, 2), work.numel() - 8,
               None) == A.DEMOD_BAD_ARG
    assert mod(d._h, ref(x), p(state), p(ring), p(cnt), S, p(pcm), p(work), work.numel() - 9, None) == A.DEMOD_BAD_ARG
    bad = tx_cfg(A, c)
    bad.max_samples = 2884
    assert mod(d._h, ref(bad), p(state), p(ring), p(cnt), S, p(pcm), p(work), work.numel(), None) == A.DEMOD_BAD_ARG
    torch.cuda.synchronize()
    with pytest.raises(A.DemodError):       # the Python mirror: a short tensor
        d.tx_modulate_async(x, state, ring, cnt, S, pcm[:100], work)


# ---- the handles: loopback -----------------------------------------------------------------

def loop_run(A, torch, c, S, K, fec, datas, N, total, drops, pieces, seed):
    """One transmitter and one receiver of S streams: LOOP_LEAD samples of idle,
    the frames of every stream in one send in shuffled stream order, then the
    rest; every pull's packets, less each stream's dropped leading samples, go
    into the receiver. Returns (per stream samples, places [S][frames], frames
    [(stream, window, body)], the transmitter's states)."""
    n, hop = T.LOOP_N, T.LOOP_HOP
    ring_w = (total // hop) + 64
    rxcfg = A.make_rx_cfg(c.sync, 0, N, c.h, c.kind, fec, 8, ring_w)
    perm = np.random.default_rng(seed).permutation(S).tolist()
    order = [(s, i) for i in range(len(datas)) for s in perm]      # shuffled stream order, a stream's own kept
    pcm, got, left = [[] for _ in range(S)], [], list(drops)
    with A.Transmitter(S, tx_cfg(A, c), n=n, hop=hop, freqs=tones(K)) as tx, \
            A.Receiver(S, rxcfg, n=n, hop=hop, freqs=tones(K)) as rx:
        at, k, places = 0, 0, None
        while at < total:
            if at == T.LOOP_LEAD:
                rec = np.zeros(len(order), A.RX_FRAME_DTYPE)
                body = b""
                for j, (s, i) in enumerate(order):        # a demod_rx_frame_t list, as a push returns it
                    rec[j]["stream"], rec[j]["length"], rec[j]["body"] = s, len(datas[i]), len(body)
                    body += datas[i]
                accepted, pl = tx.send(rec, body)
                assert accepted == len(order) and (pl["status"] == T.OK).all()
                places = {si: p for si, p in zip(order, pl)}
            m = min(pieces[k % len(pieces)], (T.LOOP_LEAD if at < T.LOOP_LEAD else total) - at)
            k += 1
            out = tx.pull(m)
            packets = []
            for s in range(S):
                pcm[s].append(out[s])
                cut = min(left[s], m)
                left[s] -= cut
                packets.append(out[s][cut:] if m - cut else None)
            fr, bodies, _ = rx.push(packets)
            got += [(int(f["stream"]), int(f["window"]), b) for f, b in zip(fr, bodies)]
            at += m
        states = [tx.state(s) for s in range(S)]
        assert all(rx.state(s)["dropped"] == 0 and rx.state(s)["cut_hits"] == 0 for s in range(S))
    return [np.concatenate(p) for p in pcm], places, got, states


@pytest.mark.parametrize("fec", [0, 1])
@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("S", [1, 3, 65])
def test_loopback(A, torch, lut, S, K, fec):
    """Every accepted frame comes back once, with its bytes, at window R start
    minus the stream's dropped windows; ragged pulls give identical samples,
    which are the reference's."""
    c, datas, N, total = T.loopback_case(K, fec, lut)
    n, hop = T.LOOP_N, T.LOOP_HOP
    R = n // hop
    drops = [hop * ((3 * s) % 5) for s in range(S)]             # whole windows, below the lead
    pcm, places, got, states = loop_run(A, torch, c, S, K, fec, datas, N, total, drops, [2880], S)
    want = sorted((s, R * int(places[s, i]["start"]) - drops[s] // hop, datas[i])
                  for s in range(S) for i in range(len(datas)))
    assert sorted(got) == want
    ragged = [1, 7, 997, 2880, 8, 9, n - 1, n, n + 1, 2880, 2880, 2880]
    pcm2, places2, got2, states2 = loop_run(A, torch, c, S, K, fec, datas, N, total, drops, ragged, S)
    assert sorted(got2) == want and states2 == states
    ref, ends = T.Tx(c, S), [2880 if s in (0, S - 1) else 0 for s in range(S)]   # the first and the last stream
    lead = ref.pull(ends), ref.pull(ends)
    ref.send([(s, d) for s in (0, S - 1)[:S] for d in datas])
    rest = [ref.pull(ends) for _ in range((total - T.LOOP_LEAD) // 2880)]
    for s in range(S):
        assert np.array_equal(pcm[s], pcm2[s]), s
        if s in (0, S - 1):
            same(pcm[s], np.concatenate([p[s] for p in list(lead) + rest]), ("reference", s))
    for s in range(S):
        assert states[s]["accepted"] == len(datas) and states[s]["refused"] == 0


def test_handle_refusals_and_statuses(A, torch, lut):
    """A refused send or pull leaves every stream's state as it was; a frame
    above max_len and one without room are statuses, not refusals; reset zeroes
    one stream."""
    K, S = 2, 3
    c, datas, N, total = T.loopback_case(K, 0, lut)
    c.C = 2 * (T.frame_count(c, 3) + c.gap)
    with A.Transmitter(S, tx_cfg(A, c), n=T.LOOP_N, hop=T.LOOP_HOP, freqs=tones(K)) as tx:
        tx.pull([100, 0, 2048])
        accepted, pl = tx.send([(2, b"abc"), (0, b"1234"), (2, b"xyz"), (2, b"q")])
        assert accepted == 2 and pl["status"].tolist() == [T.OK, T.BAD_LENGTH, T.OK, T.NO_ROOM]
        ref = T.Tx(c, S)
        ref.pull([100, 0, 2048])
        assert np.array_equal(ref.send([(2, b"abc"), (0, b"1234"), (2, b"xyz"), (2, b"q")]), pl)
        before = [tx.state(s) for s in range(S)]
        assert before == [{f: int(ref.state[s][f]) for f in T.STATE_DTYPE.names} for s in range(S)]
        for frames in ([(3, b"a")], [(0, b"a")] * 4, [(-1 % 2 ** 32, b"")]):
            with pytest.raises(A.DemodError) as e:
                tx.send(frames)
            assert e.value.code == A.DEMOD_BAD_ARG
        rec = np.zeros(1, A.RX_FRAME_DTYPE)
        rec[0]["length"], rec[0]["body"] = 3, 2
        with pytest.raises(A.DemodError):
            tx.send(rec, b"abcd")                           # body + length past n_bytes
        with pytest.raises(A.DemodError):
            tx.pull([0, 2881, 0])
        with pytest.raises(A.DemodError):
            tx.pull([1, 2])
        assert [tx.state(s) for s in range(S)] == before
        tx.reset(2)
        assert tx.state(2) == {f: 0 for f in T.STATE_DTYPE.names} and tx.state(0) == before[0]
        with pytest.raises(A.DemodError):
            tx.reset(3)
    bad = tx_cfg(A, c)
    bad.ring_symbols = 10
    with pytest.raises(A.DemodError) as e:
        A.Transmitter(S, bad, n=T.LOOP_N, hop=T.LOOP_HOP, freqs=tones(K))
    assert e.value.code == A.DEMOD_BAD_ARG


# ---- reuse: the handle's samples stay on the device -----------------------------------------

def test_device_pcm_through_detector_and_scan(A, torch, handle, lut):
    """One pull whose stride is a multiple of hop; the handle's [S][stride]
    samples on the device go through demod_batch_async and
    demod_frames_segments_async with first[s] = s stride / hop: the hits are at
    R start of the planted frames."""
    import ctypes
    K, n, S = 2, 256, 3
    hop, R = n // 4, 4
    rng = np.random.default_rng(8)
    word = rng.integers(0, K, 16).astype(np.uint8)
    c = T.make(tones(K), n, lut, word, h=1, kind=C.CRC16, fec=0, max_len=3, gap=2, idle=(0, 1), amplitude=8000,
               sigma=400, seed=77, max_frames=1, stride=200 * n)
    N = X.row_symbols(1, C.CRC16, 0, 1, 3)
    datas = [b"abc", b"", b"\x00\xff"]
    d = handle(K, n)
    with A.Transmitter(S, tx_cfg(A, c), n=n, hop=hop, freqs=tones(K)) as tx:
        tx.pull([3 * n, 5 * n, 0])
        accepted, places = tx.send([(s, datas[s]) for s in range(S)])
        assert accepted == S
        heads = [tx.state(s)["head"] for s in range(S)]
        tx.pull(c.stride)
        d_pcm = tx.device_pcm()
        assert d_pcm.numel() == S * c.stride and d_pcm.dtype == torch.int16
        W = (S * c.stride - n) // hop + 1
        d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
        d_mag = torch.empty(W * K, dtype=torch.float32, device="cuda")
        d.batch_async(d_pcm, W, d_sym, d_mag)
        first = np.array([s * c.stride // hop for s in range(S)], np.int64)
        count = np.full(S, (c.stride - n) // hop + 1, np.int32)
        cap = 4
        d_hits = torch.zeros(S * cap * ctypes.sizeof(A.DemodFrameHit), dtype=torch.uint8, device="cuda")
        d_packed = torch.zeros(S * cap * ((N + 7) // 8), dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(S * ctypes.sizeof(A.DemodFramesResult), dtype=torch.uint8, device="cuda")
        d_work = torch.empty(A.frames_segments_workspace_size(d.cfg, S, W), dtype=torch.uint8, device="cuda")
        d.frames_segments_async(d_sym, d_mag, W, torch.from_numpy(first).cuda(), torch.from_numpy(count).cuda(), S,
                                word, 0, N, d_hits, None, d_packed, cap, d_res, d_work)
        torch.cuda.synchronize()
        hits = d_hits.cpu().numpy().view(C.HIT_DTYPE).reshape(S, cap)
        res = d_res.cpu().numpy().view(X.RESULT_DTYPE)
        packed = d_packed.cpu().numpy().reshape(S, cap, -1)
        for s in range(S):
            assert int(res["n_written"][s]) == 1, (s, res["n_hits"][s])
            assert int(hits["window"][s, 0]) == R * (int(places["start"][s]) - heads[s])
            assert int(packed[s, 0, 0]) == len(datas[s])
            assert packed[s, 0, 1:1 + len(datas[s])].tobytes() == datas[s]
