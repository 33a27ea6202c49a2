#!/usr/bin/env python3
"""Cost of the transmitter (include/demod.h "transmitter"), in one process,
after the method of scripts/rx_cost.py: medians with min-max.

Live shape: 1024 streams x one 2880-sample pull, n = 1024, hop 256, K = 2 and
K = 8, plain and coded frames (a 16-symbol word, a 1-byte length, CRC-16, 3
data bytes, 3 idle symbols behind each frame).
  device  demod_tx_encode_async (one frame for every stream into an empty
          queue: the states are zeroed, untimed, before every replay) and
          demod_tx_modulate_async (a frame in flight on every stream), each a
          captured graph timed by events around its replay, beside
          demod_synth_fsk on the same 2.9 M samples.
  host    the time around demod_tx_pull beside demod_rx_push on the same
          packets, after --warmup rounds (the longest frame, 160 symbols at
          K = 2 coded, spans 57 packets); every stream is sent a frame whenever
          its queue holds less than one.

Offline shape: 64 streams x 2^20 samples and 1 stream x 2^26 samples, K = 2, a
full queue behind every stream (states and rings written directly): the whole
modulate call by events beside demod_synth_fsk at the same sample count, and
the phase, samples and state launches one by one from torch.profiler's kernel
records (null when the profiler has none).

    python scripts/tx_cost.py [--streams 1024] [--reps 40] [--skip-offline]

Prints one JSON line. Needs an MI355X: there is no CPU path.
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load_pkg():
    spec = importlib.util.spec_from_file_location(
        "audio_network_amd", os.path.join(ROOT, "audio-network_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["audio_network_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def mmm(v):
    """median [min, max], microseconds"""
    return [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]


def timed(torch, fn, reps, before=None):
    """Event time of fn() in microseconds, reps times after two untimed runs."""
    out = []
    for i in range(reps + 2):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= 2:
            out.append(e0.elapsed_time(e1) * 1e3)
    return out


def graph_of(torch, step):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step(side.cuda_stream)          # eager first: the sine table goes up outside the capture
        side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step(torch.cuda.current_stream().cuda_stream)
    return g


def kernel_times(torch, fn, reps, names):
    """Median device time (us) of the kernels whose name holds one of `names`, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        got = {k: [] for k in names}
        for ev in prof.events():
            for k in names:
                if k in ev.name:
                    t = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
                    if t:
                        got[k].append(float(t))
        return {k: mmm(v) for k, v in got.items()} if all(got.values()) else None
    except Exception as e:      # a measurement aid, not a code path of the library
        return {"error": repr(e)[:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=80)
    ap.add_argument("--skip-offline", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("tx_cost.py: no GPU visible (nothing is measured without one)")
    A = load_pkg()
    import rx_ref as X       # the receiver's row width for the tests' frame formats
    lib = A.load_library()
    n, hop, packet, S, L, h, kind = 1024, 256, 2880, args.streams, 16, 1, A.DEMOD_CRC16_CCITT_FALSE
    R = n // hop
    out = {"streams": S, "pull_samples": packet, "n": n, "hop": hop, "reps": args.reps}
    u8 = lambda nb: torch.zeros(nb, dtype=torch.uint8, device="cuda")

    for K in (2, 8):
        freqs = tuple(1500.0 + 375.0 * i for i in range(K))
        bits = A.bits_per_symbol(K)
        cfg = A.make_cfg(n=n, hop=hop, freqs=freqs)
        for fec in (0, A.DEMOD_FEC_CONV_K7):
            rng = np.random.default_rng(K + fec)
            word = rng.integers(0, K, L).astype(np.uint8)
            x = A.make_tx_cfg(word, h, kind, fec, 3, 3, (0, 1), 8000, 400, 7, 0, 1, packet)
            a = A.tx_frame_symbol_count(x, K, 3) + 3
            x.ring_symbols = 2 * a
            z = A.tx_sizes(cfg, x, S)
            N = X.row_symbols(h, kind, fec, bits, 3)
            res = {"frame_symbols": a - 3, "ring_symbols": int(x.ring_symbols)}
            # ---- device stages as graphs
            with A.Demodulator(cfg) as d:
                d_state, d_ring = u8(z["state_bytes"]), u8(z["ring_bytes"])
                rec = np.zeros((S, 1), A.TX_RECORD_DTYPE)
                rec["length"], rec["body"][:, 0] = 3, 3 * np.arange(S)
                d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
                d_one = torch.ones(S, dtype=torch.int32, device="cuda")
                d_bytes = torch.from_numpy(rng.integers(0, 256, 3 * S).astype(np.uint8)).cuda()
                d_place = u8(z["places_bytes"])
                d_cnt = torch.full((S,), packet, dtype=torch.int32, device="cuda")
                d_pcm = torch.zeros(S * packet, dtype=torch.int16, device="cuda")
                d_work = u8(z["modulate_work_bytes"])
                g_enc = graph_of(torch, lambda st: d.tx_encode_async(x, d_state, d_ring, d_rec, d_one, d_bytes,
                                                                     3 * S, S, d_place, stream=st))
                g_mod = graph_of(torch, lambda st: d.tx_modulate_async(x, d_state, d_ring, d_cnt, S, d_pcm, d_work,
                                                                       stream=st))
                res["encode_graph_us"] = mmm(timed(torch, g_enc.replay, args.reps, before=d_state.zero_))

                def refill():       # a frame in flight on every stream at every timed replay
                    d_state.zero_()
                    g_enc.replay()
                res["modulate_graph_us"] = mmm(timed(torch, g_mod.replay, args.reps, before=refill))
                W = S * packet // n
                res["synth_fsk_us"] = mmm(timed(
                    torch, lambda: A.synth_fsk(cfg, 7, W, 8000, 400, d_pcm[:W * n]), args.reps))
            # ---- host calls
            rxcfg = A.make_rx_cfg(word, 0, N, h, kind, fec, 4, 2 * (L + N) * R)
            kw = dict(n=n, hop=hop, freqs=freqs)
            buf = np.zeros((S, packet), np.int16)
            ptrs = (buf.ctypes.data + 2 * packet * np.arange(S)).astype(np.uintp)
            nfr = np.full(S, packet, np.uintp)
            fr, bo, su = ctypes.c_void_p(), ctypes.c_void_p(), A.DemodRxSummary()
            frames = np.zeros(S, A.RX_FRAME_DTYPE)
            frames["stream"], frames["length"], frames["body"] = np.arange(S), 3, 3 * np.arange(S)
            bodies = rng.integers(0, 256, 3 * S).astype(np.uint8)
            t_pull, t_push, t_send, n_frames, sent = [], [], [], 0, 0
            with A.Transmitter(S, x, **kw) as tx, A.Receiver(S, rxcfg, **kw) as rx:
                for i in range(args.warmup + args.reps):
                    st = tx.state(0)
                    if st["tail"] - st["head"] <= 1:          # every stream is in step with stream 0
                        t0 = time.perf_counter()
                        rc = lib.demod_tx_send(tx._h, frames.ctypes.data, S, bodies.ctypes.data, bodies.size, None)
                        t_send.append(time.perf_counter() - t0)
                        if rc != S:
                            sys.exit(f"tx_cost.py: send accepted {rc} of {S}")
                        sent += S
                    t0 = time.perf_counter()
                    rp = lib.demod_tx_pull(tx._h, nfr.ctypes.data, ptrs.ctypes.data)
                    t1 = time.perf_counter()
                    rc = lib.demod_rx_push(rx._h, ptrs.ctypes.data, nfr.ctypes.data, ctypes.byref(fr),
                                           ctypes.byref(bo), ctypes.byref(su))
                    t2 = time.perf_counter()
                    if rp < 0 or rc < 0:
                        sys.exit(f"tx_cost.py: pull or push failed ({rp}, {rc})")
                    n_frames += rc
                    if i >= args.warmup:
                        t_pull.append((t1 - t0) * 1e6)
                        t_push.append((t2 - t1) * 1e6)
            res.update(tx_pull_us=mmm(t_pull), rx_push_us=mmm(t_push), tx_send_us=mmm([t * 1e6 for t in t_send]),
                       frames_sent=sent, frames_received=n_frames)
            out[f"k{K}_{'coded' if fec else 'plain'}"] = res

    if not args.skip_offline:
        K = 2
        freqs = (1500.0, 1875.0)
        cfg = A.make_cfg(n=n, hop=hop, freqs=freqs)
        for S2, m in ((64, 2 ** 20), (1, 2 ** 26)):
            C = m // n + 8
            x = A.make_tx_cfg([0, 1, 1, 0], h, kind, 0, 3, 0, (0, 1), 8000, 400, 7, C, 1, m)
            z = A.tx_sizes(cfg, x, S2)
            with A.Demodulator(cfg) as d:
                state = np.zeros(S2, A.TX_STATE_DTYPE)
                state["tail"] = C
                d_state = torch.from_numpy(state.view(np.uint8).copy()).cuda()
                keep = d_state.clone()
                d_ring = torch.randint(0, K, (z["ring_bytes"],), dtype=torch.uint8, device="cuda")
                d_cnt = torch.full((S2,), m, dtype=torch.int32, device="cuda")
                d_pcm = torch.zeros(S2 * m, dtype=torch.int16, device="cuda")
                d_work = u8(z["modulate_work_bytes"])
                run = lambda: d.tx_modulate_async(x, d_state, d_ring, d_cnt, S2, d_pcm, d_work)
                reset = lambda: d_state.copy_(keep)
                res = {"modulate_us": mmm(timed(torch, run, 10, before=reset))}
                W = S2 * m // n
                res["synth_fsk_us"] = mmm(timed(torch, lambda: A.synth_fsk(cfg, 7, W, 8000, 400, d_pcm), 10))

                def both():
                    reset()
                    run()
                    A.synth_fsk(cfg, 7, W, 8000, 400, d_pcm)
                res["kernels_us"] = kernel_times(torch, both, 10, ("tx_phase_kernel", "tx_samples_kernel",
                                                                   "tx_state_kernel", "synth_kernel"))
            out[f"offline_{S2}x2^{m.bit_length() - 1}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
