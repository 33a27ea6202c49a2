#!/usr/bin/env python3
"""Cost of demod_frames_async beside the detector step and demod_acquire_async
on the same buffers.

scripts/acquire_cost.py's method and shape: configs[3] (the sliding 1024-point
FFT detector, hop 256, 2-FSK, 2^20 x 1024 synthetic samples = 4 194 301
windows), device events around each enqueue on one stream, warm-up rounds, then
medians over --reps repeats with every figure taken once per round in turn, one
process. The frame scan is timed as its eager launches and as one replay of a
captured graph of them, for a 24-symbol word in four sub-cases:

  no_hit      a random word on the detector's own symbols (n_hits is printed)
  planted     ~1000 frames of 256 symbols (the word + 232 payload symbols)
              planted on the acquired phase of a copy of the symbols, payload
              and packed outputs
  count_only  no_hit with max_frames = 0 (scan + finalise)
  all_hit     K = 1, a one-symbol word, every symbol 0: every start hits
              (1 048 576 hits of 8 payload symbols)

    python scripts/frames_cost.py [--windows 1048576] [--reps 30] [--case NAME]

--case runs one sub-case's eager launches alone (for a kernel trace). Prints
one JSON line. Needs an MI355X: there is no CPU path.
"""
import argparse
import ctypes
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
    ap.add_argument("--case", choices=("no_hit", "planted", "count_only", "all_hit", "acquire"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("frames_cost.py: no GPU visible (nothing is measured without one)")
    A = load_pkg()
    n, hop, freqs = 1024, args.hop, A.FSK2_FREQS
    gen_cfg = A.make_cfg(freqs=freqs, n=n)
    cfg = A.make_cfg(freqs=freqs, n=n, hop=hop, method=A.METHOD_FFT)
    cfg1 = A.make_cfg(freqs=freqs[:1], n=n, hop=hop)
    Wg = args.windows
    W = (Wg * n - n) // hop + 1
    R, K, L, N = n // hop, len(freqs), 24, 232
    d_pcm = torch.empty((Wg, n), dtype=torch.int16, device="cuda")
    A.synth_fsk(gen_cfg, A.BENCH_SEED, Wg, 8000, 400, d_pcm, None)
    d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
    d_mag = torch.empty((W, K), dtype=torch.float32, device="cuda")
    d_ares = torch.empty(ctypes.sizeof(A.DemodAcquireResult), dtype=torch.uint8, device="cuda")
    d_awork = torch.empty(A.acquire_workspace_size(cfg), dtype=torch.uint8, device="cuda")
    d_res = torch.empty(ctypes.sizeof(A.DemodFramesResult), dtype=torch.uint8, device="cuda")
    d_work = torch.empty(A.frames_workspace_size(cfg, W), dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(1)
    word = rng.integers(0, K, L).astype(np.uint8)
    side = torch.cuda.Stream()
    out = {"windows": W, "hop": hop, "k": K, "phases": R, "method": "fft", "reps": args.reps,
           "sync_len": L, "work_bytes": int(d_work.numel())}

    def outputs(cap, n_sym, bits):
        B = (n_sym * bits + 7) // 8
        return [torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
                for nb in (cap * ctypes.sizeof(A.DemodFrameHit), cap * n_sym, cap * B)]

    with A.Demodulator(cfg) as d, A.Demodulator(cfg1) as d1, torch.cuda.stream(side):
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

        def acquire():
            d.acquire_async(d_sym, d_mag, W, word, 0, None, d_ares, d_awork, stream=s)

        def result():
            side.synchronize()
            res = A.frames_result_dict(A.DemodFramesResult.from_buffer_copy(d_res.cpu().numpy().tobytes()))
            return {f: res[f] for f in ("phase", "n_hits", "n_written", "tail_window")}

        detector()
        side.synchronize()
        d.frames_async(d_sym, d_mag, W, word, 0, N, None, None, None, 0, d_res, d_work, stream=s)
        phase = result()["phase"]
        # ~1000 frames, 4096 windows apart, on the acquired phase of a copy of the symbols
        sym_p = d_sym.cpu().numpy().copy()
        payload = rng.integers(0, K, (1000, N)).astype(np.uint8)
        for f in range(1000):
            w0 = phase + 4096 * f + 512
            sym_p[w0:w0 + L * R:R] = word
            sym_p[w0 + L * R:w0 + (L + N) * R:R] = payload[f]
        d_sym_p = torch.from_numpy(sym_p).cuda()
        cap = 2048
        hits_p, pay_p, pak_p = outputs(cap, N, 1)
        # every start hits: K = 1, every symbol 0
        d_sym0 = torch.zeros(W, dtype=torch.uint8, device="cuda")
        d_mag1 = torch.ones(W, dtype=torch.float32, device="cuda")
        cap0, N0 = W // R + 1, 8
        hits_0, pay_0, pak_0 = outputs(cap0, N0, 1)
        one = np.zeros(1, np.uint8)
        cases = {
            "no_hit": lambda: d.frames_async(d_sym, d_mag, W, word, 0, N, hits_p, pay_p, pak_p, cap, d_res,
                                             d_work, stream=s),
            "planted": lambda: d.frames_async(d_sym_p, d_mag, W, word, 0, N, hits_p, pay_p, pak_p, cap,
                                              d_res, d_work, stream=s),
            "count_only": lambda: d.frames_async(d_sym, d_mag, W, word, 0, N, None, None, None, 0, d_res,
                                                 d_work, stream=s),
            "all_hit": lambda: d1.frames_async(d_sym0, d_mag1, W, one, 0, N0, hits_0, pay_0, pak_0, cap0,
                                               d_res, d_work, stream=s),
        }
        if args.case:
            fn = acquire if args.case == "acquire" else cases[args.case]
            for _ in range(args.warmup + args.reps):
                fn()
            side.synchronize()
            out["case"] = args.case
            print(json.dumps(out))
            return
        runs = {"detector": detector, "acquire_eager": acquire}
        graphs = []
        for name, fn in [("acquire", acquire)] + list(cases.items()):
            fn()
            if name != "acquire":
                out[name + "_result"] = result()
                runs[name + "_eager"] = fn
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn()
            graphs.append(g)
            runs[name + "_graph"] = g.replay
        cases["planted"]()
        side.synchronize()
        got = pay_p.cpu().numpy()[:1000 * N].reshape(1000, N)
        out["planted_payloads_equal"] = bool(np.array_equal(got, payload))
        times = {k: [] for k in runs}
        for rep in range(args.warmup + args.reps):
            for k, fn in runs.items():
                t = timed(fn)
                if rep >= args.warmup:
                    times[k].append(t)
        for k, v in times.items():
            out[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                              "max": round(max(v), 2)}
        base = out["acquire_graph_us"]["median"]
        for name in cases:
            out[name + "_graph_over_acquire"] = round(out[name + "_graph_us"]["median"] / base, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
