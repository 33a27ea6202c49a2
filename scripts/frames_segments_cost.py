#!/usr/bin/env python3
"""Cost of demod_frames_segments_async beside what it replaces: demod_frames_async
on the same buffers (one segment), and the loop of one demod_frames_async per
segment (many segments).

scripts/frames_cost.py's method and shape: configs[3] (the sliding 1024-point
FFT detector, hop 256, 2-FSK, 2^20 x 1024 synthetic samples = 4 194 301
windows), device events around each enqueue on one stream, warm-up rounds, then
medians over --reps repeats with every figure taken once per round in turn, one
process. A 24-symbol word, 232 payload symbols, payload and packed outputs.

  (a) S = 1 over the whole batch, graph against graph of demod_frames_async:
      no_hit      a random word on the detector's own symbols
      planted     1000 frames planted on the acquired phase of a copy
      count_only  no_hit with max_frames = 0
  (b) S = 1024 segments of 11 windows (a 60 ms packet each), the detector's
      symbols: the segmented call (eager and graph) against the eager loop of
      1024 demod_frames_async calls on the slices.
  (c) S = 1024 segments of 4096 windows, three frames planted in each: the
      segmented call, eager, against the eager loop.

The segmented acquisition is timed on the same tables (its scan shares
acquire_seg_scan.h with the segmented frame scan).

    python scripts/frames_segments_cost.py [--windows 1048576] [--reps 30] [--baseline]
                                           [--case NAME]

--baseline leaves the segmented frame scan out: what remains runs on a library
that predates it (FSKD_LIB), which is how the loops' and the segmented
acquisition's figures are confirmed unchanged. --case runs one figure's eager
launches alone (for a kernel trace). Prints one JSON line. Needs an MI355X:
there is no CPU path.
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
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--case")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("frames_segments_cost.py: no GPU visible (nothing is measured without one)")
    A = load_pkg()
    n, hop, freqs = 1024, args.hop, A.FSK2_FREQS
    gen_cfg = A.make_cfg(freqs=freqs, n=n)
    cfg = A.make_cfg(freqs=freqs, n=n, hop=hop, method=A.METHOD_FFT)
    Wg = args.windows
    W = (Wg * n - n) // hop + 1
    R, K, L, N = n // hop, len(freqs), 24, 232
    B = (N + 7) // 8
    HIT, RES, ARES = (ctypes.sizeof(t) for t in (A.DemodFrameHit, A.DemodFramesResult, A.DemodAcquireResult))
    d_pcm = torch.empty((Wg, n), dtype=torch.int16, device="cuda")
    A.synth_fsk(gen_cfg, A.BENCH_SEED, Wg, 8000, 400, d_pcm, None)
    d_sym = torch.empty(W, dtype=torch.uint8, device="cuda")
    d_mag = torch.empty((W, K), dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(1)
    word = rng.integers(0, K, L).astype(np.uint8)
    side = torch.cuda.Stream()
    out = {"windows": W, "hop": hop, "k": K, "phases": R, "method": "fft", "reps": args.reps, "sync_len": L,
           "frame_symbols": N, "baseline": bool(args.baseline)}

    def u8(nbytes):
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")

    def tables(first, count):
        f = np.ascontiguousarray(first, np.uint64).view(np.int64)
        c = np.ascontiguousarray(count, np.uint32).view(np.int32)
        return torch.from_numpy(f.copy()).cuda(), torch.from_numpy(c.copy()).cuda()

    with A.Demodulator(cfg) as d, torch.cuda.stream(side):
        s = side.cuda_stream

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(side)
            fn()
            b.record(side)
            b.synchronize()
            return a.elapsed_time(b) * 1e3     # us

        def results(t, S):
            side.synchronize()
            raw = t.cpu().numpy().tobytes()
            return [A.frames_result_dict(A.DemodFramesResult.from_buffer_copy(raw[i * RES:(i + 1) * RES]))
                    for i in range(S)]

        d.batch_async(d_pcm, W, d_sym, d_mag, stream=s)
        side.synchronize()
        d_work1 = u8(A.frames_workspace_size(cfg, W))
        d_res1 = u8(RES)
        d.frames_async(d_sym, d_mag, W, word, 0, N, None, None, None, 0, d_res1, d_work1, stream=s)
        phase = results(d_res1, 1)[0]["phase"]
        sym_host = d_sym.cpu().numpy()
        # (a): 1000 frames, 4096 windows apart, on the acquired phase of a copy of the symbols
        sym_p = sym_host.copy()
        payload = rng.integers(0, K, (1000, N)).astype(np.uint8)
        for f in range(1000):
            w0 = phase + 4096 * f + 512
            sym_p[w0:w0 + L * R:R] = word
            sym_p[w0 + L * R:w0 + (L + N) * R:R] = payload[f]
        d_sym_p = torch.from_numpy(sym_p).cuda()
        # (c): three frames in each run of 4096 windows, on the same phase
        S_c = min(1024, W // 4096 + (W % 4096 >= 1100 * 3))
        first_c = [4096 * i for i in range(S_c)]
        count_c = [min(4096, W - f) for f in first_c]
        sym_c = sym_host.copy()
        for f in first_c:
            for j in range(3):
                w0 = f + phase + 1100 * j + 40
                sym_c[w0:w0 + L * R:R] = word
        d_sym_c = torch.from_numpy(sym_c).cuda()
        # (b): 1024 runs of 11 windows
        S_b = 1024
        first_b = [11 * i for i in range(S_b)]
        count_b = [11] * S_b
        cap_a, cap_b, cap_c = 2048, 2, 8
        one = dict(hits=u8(cap_a * HIT), pay=u8(cap_a * N), pak=u8(cap_a * B))
        runs, cases = {}, {}

        # the whole-batch calls and the loops: on every library
        cases["a_frames_no_hit"] = lambda: d.frames_async(d_sym, d_mag, W, word, 0, N, one["hits"], one["pay"],
                                                          one["pak"], cap_a, d_res1, d_work1, stream=s)
        cases["a_frames_planted"] = lambda: d.frames_async(d_sym_p, d_mag, W, word, 0, N, one["hits"],
                                                           one["pay"], one["pak"], cap_a, d_res1, d_work1,
                                                           stream=s)
        cases["a_frames_count_only"] = lambda: d.frames_async(d_sym, d_mag, W, word, 0, N, None, None, None, 0,
                                                              d_res1, d_work1, stream=s)

        def loop(sym_t, first, count, cap, bufs):
            mag = d_mag.reshape(-1)

            def run():
                for i, (f, c) in enumerate(zip(first, count)):
                    d.frames_async(sym_t[f:f + c], mag[f * K:(f + c) * K], c, word, 0, N,
                                   bufs["hits"][i * cap * HIT:(i + 1) * cap * HIT],
                                   bufs["pay"][i * cap * N:(i + 1) * cap * N],
                                   bufs["pak"][i * cap * B:(i + 1) * cap * B], cap,
                                   bufs["res"][i * RES:(i + 1) * RES], d_work1, stream=s)
            return run

        def seg_bufs(S, cap):
            return dict(hits=u8(S * cap * HIT), pay=u8(S * cap * N), pak=u8(S * cap * B), res=u8(S * RES))

        loop_b, loop_c = seg_bufs(S_b, cap_b), seg_bufs(S_c, cap_c)
        cases["b_loop"] = loop(d_sym, first_b, count_b, cap_b, loop_b)
        cases["c_loop"] = loop(d_sym_c, first_c, count_c, cap_c, loop_c)

        # the segmented acquisition on the same tables
        tab = {"a": tables([0], [W]), "b": tables(first_b, count_b), "c": tables(first_c, count_c)}
        nseg = {"a": 1, "b": S_b, "c": S_c}
        syms = {"a": d_sym, "b": d_sym, "c": d_sym_c}
        d_ares = u8(1024 * ARES)
        d_awork = u8(A.acquire_segments_workspace_size(cfg, 1024, W))
        for k in ("a", "b", "c"):
            cases[k + "_acquire_segments"] = (lambda k=k: d.acquire_segments_async(
                syms[k], d_mag, W, tab[k][0], tab[k][1], nseg[k], word, 0, None, d_ares, d_awork, stream=s))

        graphed = ["a_frames_no_hit", "a_frames_planted", "a_frames_count_only", "a_acquire_segments",
                   "b_acquire_segments", "c_acquire_segments"]
        eager = ["b_loop", "c_loop", "b_acquire_segments", "c_acquire_segments"]
        if not args.baseline:
            d_swork = u8(A.frames_segments_workspace_size(cfg, 1024, W))
            seg_a = seg_bufs(1, cap_a)
            seg_b, seg_c = seg_bufs(S_b, cap_b), seg_bufs(S_c, cap_c)

            def seg(k, sym_t, cap, bufs, count_only=False):
                def run():
                    d.frames_segments_async(sym_t, d_mag, W, tab[k][0], tab[k][1], nseg[k], word, 0, N,
                                            None if count_only else bufs["hits"],
                                            None if count_only else bufs["pay"],
                                            None if count_only else bufs["pak"], 0 if count_only else cap,
                                            bufs["res"], d_swork, stream=s)
                return run
            cases["a_segments_no_hit"] = seg("a", d_sym, cap_a, seg_a)
            cases["a_segments_planted"] = seg("a", d_sym_p, cap_a, seg_a)
            cases["a_segments_count_only"] = seg("a", d_sym, cap_a, seg_a, True)
            cases["b_segments"] = seg("b", d_sym, cap_b, seg_b)
            cases["c_segments"] = seg("c", d_sym_c, cap_c, seg_c)
            graphed += ["a_segments_no_hit", "a_segments_planted", "a_segments_count_only", "b_segments"]
            eager += ["b_segments", "c_segments"]

        if args.case:
            for _ in range(args.warmup + args.reps):
                cases[args.case]()
            side.synchronize()
            out["case"] = args.case
            print(json.dumps(out))
            return

        # the segmented call's outputs are the loop's, byte for byte
        if not args.baseline:
            for k, lb, sb, S in (("b", loop_b, seg_b, S_b), ("c", loop_c, seg_c, S_c)):
                for t in list(lb.values()) + list(sb.values()):
                    t.fill_(0xFF)
                cases[k + "_loop"]()
                cases[k + "_segments"]()
                side.synchronize()
                out[k + "_equal_loop"] = all(bool(torch.equal(lb[f], sb[f])) for f in ("hits", "pay", "pak"))
                res = results(sb["res"], S)
                out[k + "_n_hits"] = int(sum(r["n_hits"] for r in res))
                out[k + "_segments"] = S
            for t in list(one.values()) + list(seg_a.values()):
                t.fill_(0xFF)
            cases["a_frames_planted"]()
            ref = results(d_res1, 1)[0]
            ref_hits = one["hits"].clone()
            cases["a_segments_planted"]()
            got = results(seg_a["res"], 1)[0]
            out["a_planted_n_hits"] = [int(ref["n_hits"]), int(got["n_hits"])]
            out["a_planted_equal"] = bool(torch.equal(ref_hits, seg_a["hits"]) and torch.equal(one["pay"], seg_a["pay"]))
        graphs = []
        for name in graphed:
            cases[name]()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                cases[name]()
            graphs.append(g)
            runs[name + "_graph"] = g.replay
        for name in eager:
            runs[name + "_eager"] = cases[name]
        times = {k: [] for k in runs}
        for rep in range(args.warmup + args.reps):
            for k, fn in runs.items():
                t = timed(fn)
                if rep >= args.warmup:
                    times[k].append(t)
        for k, v in times.items():
            out[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                              "max": round(max(v), 2)}
        if not args.baseline:
            for c in ("no_hit", "planted", "count_only"):
                out[f"a_{c}_segments_over_frames"] = round(
                    out[f"a_segments_{c}_graph_us"]["median"] / out[f"a_frames_{c}_graph_us"]["median"], 3)
            for k in ("b", "c"):
                out[f"{k}_loop_over_segments"] = round(
                    out[f"{k}_loop_eager_us"]["median"] / out[f"{k}_segments_eager_us"]["median"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
