#!/usr/bin/env python3
"""Cost of demod_acquire_async beside the detector step of the same batch.

configs[3]'s shape by default: the sliding 1024-point FFT detector, hop 256,
2-FSK, over 2^20 x 1024 synthetic samples = 4 194 301 windows. Both are timed
in this process with device events around each enqueue on one stream, after
warm-up; the figures are medians over --reps repeats, taken alternately
(detector, acquisition, detector, ..). The acquisition is timed as its eager
launches and as one replay of a captured graph of them, without a sync word
and with a 24-symbol word (found early, and absent: every window compared).

    python scripts/acquire_cost.py [--windows 1048576] [--hop 256] [--reps 30]

Prints one JSON line. Needs an MI355X: there is no CPU path.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_pkg():
    spec = importlib.util.spec_from_file_location(
        "audio_network_amd", os.path.join(ROOT, "audio-network_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["audio_network_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1 << 20, help="1024-sample windows of input")
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import ctypes

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("acquire_cost.py: no GPU visible (nothing is measured without one)")
    A = load_pkg()
    n, hop, freqs = 1024, args.hop, A.FSK2_FREQS
    gen_cfg = A.make_cfg(freqs=freqs, n=n)
    cfg = A.make_cfg(freqs=freqs, n=n, hop=hop, method=A.METHOD_FFT)
    Wg = args.windows
    W = (Wg * n - n) // hop + 1
    R, K = n // hop, len(freqs)
    d_pcm = torch.empty((Wg, n), dtype=torch.int16, device="cuda")
    d_true = torch.empty(Wg, dtype=torch.uint8, device="cuda")
    A.synth_fsk(gen_cfg, A.BENCH_SEED, Wg, 8000, 400, d_pcm, d_true)
    d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
    d_mag = torch.empty((W, K), dtype=torch.float32, device="cuda")
    d_out = torch.empty(W // R + 1, dtype=torch.uint8, device="cuda")
    d_res = torch.empty(ctypes.sizeof(A.DemodAcquireResult), dtype=torch.uint8, device="cuda")
    d_work = torch.empty(A.acquire_workspace_size(cfg), dtype=torch.uint8, device="cuda")
    truth = d_true.cpu().numpy()
    words = {"no_word": None, "word_found": truth[5:29].copy(),
             # 24 random bits: a word the stream should not hold (its result is printed)
             "word_absent": np.random.default_rng(1).integers(0, K, 24).astype(np.uint8)}
    side = torch.cuda.Stream()
    out = {"windows": W, "hop": hop, "k": K, "phases": R, "method": "fft", "reps": args.reps,
           "bytes_read": W * (1 + 4 * K)}
    with A.Demodulator(cfg) as d, torch.cuda.stream(side):
        s = side.cuda_stream

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(side)
            fn()
            b.record(side)
            b.synchronize()
            return a.elapsed_time(b) * 1e3     # us

        def detector():
            d.batch_async(d_pcm, W, d_sym, d_mag, stream=s)

        def acquire_of(word, out_t=d_out):
            return lambda: d.acquire_async(d_sym, d_mag, W, word, 0, out_t, d_res, d_work, stream=s)

        runs = {"detector": detector}
        graphs = []
        detector()
        for name, word in words.items():
            fn = acquire_of(word)
            fn()
            side.synchronize()
            res = A.acquire_result_dict(A.DemodAcquireResult.from_buffer_copy(d_res.cpu().numpy().tobytes()))
            out[name + "_result"] = {f: res[f] for f in ("phase", "sync_window", "n_out")}
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                acquire_of(word)()
            graphs.append(g)
            runs[name + "_eager"] = fn
            runs[name + "_graph"] = g.replay
        runs["no_word_no_output_eager"] = acquire_of(None, None)   # scan + finalise: no gather launch
        times = {k: [] for k in runs}
        for rep in range(args.warmup + args.reps):
            for k, fn in runs.items():
                t = timed(fn)
                if rep >= args.warmup:
                    times[k].append(t)
        for k, v in times.items():
            out[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                              "max": round(max(v), 2)}
        det = out["detector_us"]["median"]
        for name in words:
            out[name + "_graph_over_detector"] = round(out[name + "_graph_us"]["median"] / det, 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
