#!/usr/bin/env python3
"""Cost of one demod_rx_push beside demod_streams_push on the same packets, in
one process.

1024 streams x one 2880-frame packet (60 ms at 48 kHz) a push, n = 1024, hop
256, K = 2 and K = 8, plain and coded frames. Every stream carries frames back
to back (a 16-symbol word, a 1-byte length, CRC-16, 3 data bytes), so a frame is
in flight on every stream at every push; the streams read one recording at
offsets 90 samples apart, so their frames complete in different pushes. The
receiver runs with max_frames = 4 and ring_windows at its minimum.

Both calls are synchronous, so each is timed on the host around the C call
alone (the packet tables are built beforehand): after --warmup pushes (80 by
default: the longest frame, 160 symbols at K = 2 coded, spans 57 packets, and
the last stream meets its first whole frame 32 packets in, so every shape
completes frames in the timed pushes), the median over --reps pushes, the
handles taking the same packet in turn.
demod_streams_push is timed returning symbols only and, on a second handle,
symbols and powers.

    python scripts/rx_cost.py [--streams 1024] [--reps 40]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=80)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("rx_cost.py: no GPU visible (nothing is measured without one)")
    A = load_pkg()
    import rx_ref as X       # the frame encoders and the FSK signal of the tests
    n, hop, packet, S, L, h, kind, step = 1024, 256, 2880, args.streams, 16, 1, A.DEMOD_CRC16_CCITT_FALSE, 90
    pushes = args.warmup + args.reps
    total = pushes * packet
    out = {"streams": S, "packet_frames": packet, "n": n, "hop": hop, "reps": args.reps, "max_frames": 4}
    lib = A.load_library()
    for K in (2, 8):
        freqs = tuple(1500.0 + 375.0 * i for i in range(K))
        bits = A.bits_per_symbol(K)
        for fec in (0, A.DEMOD_FEC_CONV_K7):
            rng = np.random.default_rng(K + fec)
            word = rng.integers(0, K, L).astype(np.uint8)
            N = X.row_symbols(h, kind, fec, bits, 3)
            need = (S * step + total) // n + 2
            symbols = []
            while sum(map(len, symbols)) < need:
                symbols.append(X.frame_symbols(rng.integers(0, 256, 3).astype(np.uint8).tobytes(), word, bits, h,
                                               kind, fec))
            base = X.synth_pcm(freqs, np.concatenate(symbols)[:need], n, 7)
            rows = np.lib.stride_tricks.as_strided(base, (S, total), (2 * step, 2), writeable=False)
            R = n // hop
            rxcfg = A.make_rx_cfg(word, 0, N, h, kind, fec, 4, 2 * (L + N) * R)
            kw = dict(n=n, hop=hop, freqs=freqs)
            nfr = np.full(S, packet, np.uintp)
            cap = S * (packet // hop + R)
            sym = np.empty(cap, np.uint8)
            mag = np.empty((cap, K), np.float32)
            counts = np.zeros(S, np.uint32)
            fr, bo, su = ctypes.c_void_p(), ctypes.c_void_p(), A.DemodRxSummary()
            t_rx, t_st, t_sm, n_frames = [], [], [], 0
            with A.Receiver(S, rxcfg, **kw) as rx, A.Streams(S, **kw) as st, A.Streams(S, **kw) as sm:
                for i in range(pushes):
                    ptrs = (rows.ctypes.data + 2 * i * packet + 2 * step * np.arange(S)).astype(np.uintp)
                    t0 = time.perf_counter()
                    rc = lib.demod_rx_push(rx._h, ptrs.ctypes.data, nfr.ctypes.data, ctypes.byref(fr),
                                           ctypes.byref(bo), ctypes.byref(su))
                    t1 = time.perf_counter()
                    rs = lib.demod_streams_push(st._h, ptrs.ctypes.data, nfr.ctypes.data, sym.ctypes.data, None,
                                                cap, counts.ctypes.data)
                    t2 = time.perf_counter()
                    rm = lib.demod_streams_push(sm._h, ptrs.ctypes.data, nfr.ctypes.data, sym.ctypes.data,
                                                mag.ctypes.data, cap, counts.ctypes.data)
                    t3 = time.perf_counter()
                    if rc < 0 or rs < 0 or rm < 0:
                        sys.exit(f"rx_cost.py: push failed ({rc}, {rs}, {rm})")
                    if i >= args.warmup:
                        t_rx.append(t1 - t0)
                        t_st.append(t2 - t1)
                        t_sm.append(t3 - t2)
                        n_frames += rc
                states = [rx.state(s) for s in (0, S // 2, S - 1)]
            a, b, c = (statistics.median(t) * 1e6 for t in (t_rx, t_st, t_sm))
            out[f"k{K}_{'coded' if fec else 'plain'}"] = {
                "frame_symbols": N, "ring_windows": int(rxcfg.ring_windows), "rx_push_us": round(a, 1),
                "streams_push_us": round(b, 1), "streams_push_mags_us": round(c, 1),
                "ratio": round(a / b, 2), "ratio_mags": round(a / c, 2),
                "frames_per_push": round(n_frames / args.reps, 1),
                "dropped": sum(s["dropped"] for s in states), "cut_hits": sum(s["cut_hits"] for s in states)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
