#!/usr/bin/env python3
"""Cost of demod_acquire_segments_async beside demod_acquire_async and the
detector step, with scripts/acquire_cost.py's method: device events around
each enqueue on one stream, --warmup rounds, then medians over --reps rounds,
every figure taken once per round in turn, all in this process.

 (a) one whole-batch segment: S = 1 over configs[3]'s batch (the sliding
     1024-point FFT detector, hop 256, 2-FSK, 2^20 x 1024 samples = 4 194 301
     windows) against demod_acquire_async on the same buffers.
 (b) per-stream acquisition: S = 1024 segments against a loop of 1024
     demod_acquire_async calls on the same slices (raw library calls with the
     pointers worked out beforehand, so the loop pays no Python checks),
       short: one demod_streams_push-shaped batch, 1024 runs of 11 windows at
              hop 256 laid out by demod_segments_layout (14 336 windows);
       long:  1024 touching segments of 4096 windows of (a)'s batch.
     Each with a 24-symbol word, and as a fraction of its batch's detector step.

    python scripts/acquire_segments_cost.py [--windows 1048576] [--reps 30]

Prints one JSON line. Needs an MI355X: there is no CPU path.
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
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("acquire_segments_cost.py: no GPU visible (nothing is measured without one)")
    A = load_pkg()
    lib = A.load_library()
    n, hop, freqs = 1024, 256, A.FSK2_FREQS
    R, K, S = n // hop, len(freqs), args.streams
    RES = ctypes.sizeof(A.DemodAcquireResult)
    gen_cfg = A.make_cfg(freqs=freqs, n=n)
    cfg = A.make_cfg(freqs=freqs, n=n, hop=hop, method=A.METHOD_FFT)
    Wg = args.windows
    W = (Wg * n - n) // hop + 1
    d_pcm = torch.empty((Wg, n), dtype=torch.int16, device="cuda")
    d_true = torch.empty(Wg, dtype=torch.uint8, device="cuda")
    A.synth_fsk(gen_cfg, A.BENCH_SEED, Wg, 8000, 400, d_pcm, d_true)
    truth = d_true.cpu().numpy()
    word = truth[5:29].copy()
    d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
    d_mag = torch.empty((W, K), dtype=torch.float32, device="cuda")

    def tables(first, count):
        f = np.ascontiguousarray(first, np.uint64).view(np.int64)
        c = np.ascontiguousarray(count, np.uint32).view(np.int32)
        return torch.from_numpy(f.copy()).cuda(), torch.from_numpy(c.copy()).cuda()

    # (b) short: S runs of 11 windows, as demod_streams_push lays them out
    run_samples = n + 10 * hop
    s_first, s_count, Ws = A.segments_layout(cfg, [run_samples] * S)
    d_pcm_s = d_pcm.reshape(-1)[:(Ws - 1) * hop + n]
    d_sym_s = torch.empty(Ws, dtype=torch.uint8, device="cuda")
    d_mag_s = torch.empty((Ws, K), dtype=torch.float32, device="cuda")
    # (b) long: S touching segments of 4096 windows of (a)'s batch (the last one cut by the batch)
    seg = 4096
    l_first = np.arange(S, dtype=np.uint64) * seg
    l_first = l_first[l_first + R <= W]
    l_count = np.minimum(seg, W - l_first).astype(np.uint32)
    shapes = {
        "whole": (d_sym, d_mag, W, np.zeros(1, np.uint64), np.array([W], np.uint32)),
        "short": (d_sym_s, d_mag_s, Ws, s_first, s_count),
        "long": (d_sym, d_mag, W, l_first, l_count),
    }
    side = torch.cuda.Stream()
    out = {"windows": W, "hop": hop, "k": K, "phases": R, "method": "fft", "reps": args.reps,
           "short_windows": Ws, "streams": S}
    keep = []
    with A.Demodulator(cfg) as d, torch.cuda.stream(side):
        s = side.cuda_stream

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(side)
            fn()
            b.record(side)
            b.synchronize()
            return a.elapsed_time(b) * 1e3     # us

        runs = {"detector": lambda: d.batch_async(d_pcm, W, d_sym, d_mag, stream=s),
                "detector_short": lambda: d.batch_async(d_pcm_s, Ws, d_sym_s, d_mag_s, stream=s)}
        runs["detector"]()
        runs["detector_short"]()
        d_work1 = torch.empty(A.acquire_workspace_size(cfg), dtype=torch.uint8, device="cuda")
        for name, (t_sym, t_mag, Wb, first, count) in shapes.items():
            Sn = len(first)
            cap = int(count.max()) // R + 1
            d_first, d_count = tables(first, count)
            d_out = torch.empty(Sn * cap, dtype=torch.uint8, device="cuda")
            d_res = torch.empty(Sn * RES, dtype=torch.uint8, device="cuda")
            d_work = torch.empty(A.acquire_segments_workspace_size(cfg, Sn, Wb), dtype=torch.uint8,
                                 device="cuda")
            keep += [d_first, d_count, d_out, d_res, d_work]

            def segmented(w, out_t=d_out, a=(t_sym, t_mag, Wb, d_first, d_count, Sn), r=d_res, k=d_work):
                return lambda: d.acquire_segments_async(*a, w, 0, out_t, r, k, stream=s)

            # the loop: one demod_acquire_async per slice, pointers worked out beforehand
            d_res1 = torch.empty(Sn * RES, dtype=torch.uint8, device="cuda")
            d_out1 = torch.empty(Sn * cap, dtype=torch.uint8, device="cuda")
            keep += [d_res1, d_out1]
            calls = [(t_sym.data_ptr() + int(f), t_mag.data_ptr() + 4 * K * int(f), int(c),
                      d_out1.data_ptr() + i * cap, d_res1.data_ptr() + i * RES)
                     for i, (f, c) in enumerate(zip(first, count))]

            def loop(w, calls=calls):
                wp, wl = (w.ctypes.data, w.size) if w is not None else (None, 0)

                def go():
                    for ps, pm, c, po, pr in calls:
                        rc = lib.demod_acquire_async(d._h, ps, pm, c, wp, wl, 0, po, cap, pr,
                                                     d_work1.data_ptr(), s)
                        assert rc == 0, rc
                return go

            for wname, w in (("no_word", None), ("word", word)):
                fn = segmented(w)
                fn()
                loop(w)()
                side.synchronize()
                # the two agree on every integer field of every segment (the metric's sum order differs)
                a = np.frombuffer(d_res.cpu().numpy().tobytes(), np.uint8).reshape(Sn, RES)[:, 512:]
                b = np.frombuffer(d_res1.cpu().numpy().tobytes(), np.uint8).reshape(Sn, RES)[:, 512:]
                assert np.array_equal(a, b), (name, wname)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    segmented(w)()
                keep.append(g)
                runs[f"{name}_{wname}_segments_eager"] = fn
                runs[f"{name}_{wname}_segments_graph"] = g.replay
                runs[f"{name}_{wname}_loop"] = loop(w)
                if Sn == 1:      # (a): demod_acquire_async as a captured graph, too
                    g1 = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g1, stream=side):
                        lib.demod_acquire_async(d._h, *calls[0][:3], w.ctypes.data if w is not None else None,
                                                0 if w is None else w.size, 0, calls[0][3], cap, calls[0][4],
                                                d_work1.data_ptr(), torch.cuda.current_stream().cuda_stream)
                    keep.append(g1)
                    runs[f"{name}_{wname}_loop_graph"] = g1.replay
            runs[f"{name}_no_word_no_output_segments_eager"] = segmented(None, None)
            res0 = A.acquire_result_dict(A.DemodAcquireResult.from_buffer_copy(
                d_res.cpu().numpy().tobytes()[:RES]))
            out[name + "_segment0"] = {f: res0[f] for f in ("phase", "sync_window", "n_out")}
        times = {k: [] for k in runs}
        for rep in range(args.warmup + args.reps):
            for k, fn in runs.items():
                t = timed(fn)
                if rep >= args.warmup:
                    times[k].append(t)
        for k, v in times.items():
            out[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                              "max": round(max(v), 2)}
        for name in shapes:
            det = out["detector_short_us" if name == "short" else "detector_us"]["median"]
            for wname in ("no_word", "word"):
                g = out[f"{name}_{wname}_segments_graph_us"]["median"]
                out[f"{name}_{wname}_graph_over_detector"] = round(g / det, 5)
                out[f"{name}_{wname}_loop_over_segments_eager"] = round(
                    out[f"{name}_{wname}_loop_us"]["median"]
                    / out[f"{name}_{wname}_segments_eager_us"]["median"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
