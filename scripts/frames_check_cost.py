#!/usr/bin/env python3
"""Cost of demod_frames_check_async beside the frame scan it follows, on the
same buffers.

scripts/frames_cost.py's method: configs[3] (the sliding 1024-point FFT
detector, hop 256, 2-FSK, 2^20 x 1024 synthetic samples = 4 194 301 windows),
device events around each replay on one stream, warm-up rounds, then medians
over --reps repeats with every figure taken once per round in turn, one
process. Each call is timed as one replay of a captured graph of its launches.
Checked frames of a 24-symbol word, a 2-byte length and CRC-32 are planted on
the acquired phase of a copy of the detector's symbols:

  batch     1000 frames (0 .. 110 data bytes) 4096 windows apart, rows of
            N = 2048 symbols (B = 256, max_len = 250): demod_frames_async
            (hits and packed rows) against demod_frames_check_async with
            n_groups = 1, with and without d_body
  segments  1024 segments x 4096 windows with three frames each, rows of N =
            232 symbols (B = 29, max_len = 23), 8 rows a segment:
            demod_frames_segments_async against demod_frames_check_async with
            n_groups = 1024

    python scripts/frames_check_cost.py [--windows 1048576] [--reps 30] [--case NAME]

--case runs one call's eager launches alone (for a kernel trace). Prints one
JSON line. Needs an MI355X: there is no CPU path.
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--case", choices=("batch_scan", "batch_check", "segments_scan", "segments_check"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("frames_check_cost.py: no GPU visible (nothing is measured without one)")
    A = load_pkg()
    n, hop, freqs = 1024, 256, A.FSK2_FREQS
    gen_cfg = A.make_cfg(freqs=freqs, n=n)
    cfg = A.make_cfg(freqs=freqs, n=n, hop=hop, method=A.METHOD_FFT)
    Wg = args.windows
    W = (Wg * n - n) // hop + 1
    R, K, L, h, kind = n // hop, len(freqs), 24, 2, A.DEMOD_CRC32_MPEG2
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_pcm = torch.empty((Wg, n), dtype=torch.int16, device="cuda")
    A.synth_fsk(gen_cfg, A.BENCH_SEED, Wg, 8000, 400, d_pcm, None)
    d_sym = torch.empty(W, **u8)
    d_mag = torch.empty((W, K), dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(1)
    word = rng.integers(0, K, L).astype(np.uint8)
    side = torch.cuda.Stream()
    out = {"windows": W, "hop": hop, "k": K, "phases": R, "method": "fft", "reps": args.reps, "sync_len": L,
           "len_bytes": h, "crc": "crc32_mpeg2"}

    def frame_symbols_of(data):
        frame = A.checked_frame_encode(data, h, kind)
        return A.unpack_symbols(frame, len(frame) * 8, 1)

    def outputs(rows, B):
        max_len = B - h - 4
        return dict(check=torch.empty(rows * ctypes.sizeof(A.DemodFrameCheck), **u8),
                    kept=torch.empty(rows, dtype=torch.int32, device="cuda"),
                    body=torch.empty(rows * max_len, **u8),
                    summary=torch.empty(32 * 1024, **u8))     # up to 1024 groups

    with A.Demodulator(cfg) as d, torch.cuda.stream(side):
        s = side.cuda_stream

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(side)
            fn()
            b.record(side)
            b.synchronize()
            return a.elapsed_time(b) * 1e3     # us

        d.batch_async(d_pcm, W, d_sym, d_mag, stream=s)
        side.synchronize()
        d_res = torch.empty(ctypes.sizeof(A.DemodFramesResult), **u8)
        d_work = torch.empty(A.frames_workspace_size(cfg, W), **u8)
        d.frames_async(d_sym, d_mag, W, word, 0, 0, None, None, None, 0, d_res, d_work, stream=s)
        side.synchronize()
        phase = A.frames_result_dict(A.DemodFramesResult.from_buffer_copy(d_res.cpu().numpy().tobytes()))["phase"]
        base = d_sym.cpu().numpy()

        # batch: 1000 frames 4096 windows apart, rows of 2048 symbols
        n_frames = min(1000, (W - 16384) // 4096)
        N1, cap1 = 2048, 2048
        B1 = N1 // 8
        sym1 = base.copy()
        datas = [rng.integers(0, 256, int(rng.integers(0, 111))).astype(np.uint8).tobytes()
                 for _ in range(n_frames)]
        for f, data in enumerate(datas):
            w0 = phase + 4096 * f + 512
            seq = np.concatenate([word, frame_symbols_of(data)])
            sym1[w0:w0 + len(seq) * R:R] = seq
        d_sym1 = torch.from_numpy(sym1).cuda()
        hits1, packed1 = torch.empty(cap1 * 16, **u8), torch.empty(cap1 * B1, **u8)
        o1 = outputs(cap1, B1)

        # segments: 1024 x 4096 windows, three frames each, rows of 232 symbols
        S, N2, cap2 = min(1024, -(-W // 4096)), 232, 8
        B2 = N2 // 8
        first = np.arange(S, dtype=np.int64) * 4096
        count = np.minimum(4096, W - first).astype(np.int32)
        sym2 = base.copy()
        datas2 = [[rng.integers(0, 256, int(rng.integers(0, 24))).astype(np.uint8).tobytes() for _ in range(3)]
                  for _ in range(S)]
        for g in range(S):
            for f, data in enumerate(datas2[g]):
                w0 = int(first[g]) + phase + 256 + 1280 * f
                seq = np.concatenate([word, frame_symbols_of(data)])
                sym2[w0:w0 + len(seq) * R:R] = seq
        d_sym2 = torch.from_numpy(sym2).cuda()
        d_first, d_count = torch.from_numpy(first).cuda(), torch.from_numpy(count).cuda()
        hits2, packed2 = torch.empty(S * cap2 * 16, **u8), torch.empty(S * cap2 * B2, **u8)
        d_res2 = torch.empty(S * ctypes.sizeof(A.DemodFramesResult), **u8)
        d_work2 = torch.empty(A.frames_segments_workspace_size(cfg, S, W), **u8)
        o2 = outputs(S * cap2, B2)

        def check1(body=True):
            d.frames_check_async(hits1, packed1, d_res, 1, cap1, L, N1, h, kind, o1["check"], o1["kept"],
                                 o1["body"] if body else None, o1["summary"], stream=s)

        cases = {
            "batch_scan": lambda: d.frames_async(d_sym1, d_mag, W, word, 0, N1, hits1, None, packed1, cap1, d_res,
                                                 d_work, stream=s),
            "batch_check": check1,
            "batch_check_no_body": lambda: check1(False),
            "segments_scan": lambda: d.frames_segments_async(d_sym2, d_mag, W, d_first, d_count, S, word, 0, N2,
                                                             hits2, None, packed2, cap2, d_res2, d_work2,
                                                             stream=s),
            "segments_check": lambda: d.frames_check_async(hits2, packed2, d_res2, S, cap2, L, N2, h, kind,
                                                           o2["check"], o2["kept"], o2["body"], o2["summary"],
                                                           stream=s),
        }
        if args.case:
            cases[args.case.split("_")[0] + "_scan"]()
            for _ in range(args.warmup + args.reps):
                cases[args.case]()
            side.synchronize()
            out["case"] = args.case
            print(json.dumps(out))
            return
        runs = {}
        graphs = []
        for name, fn in cases.items():
            fn()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn()
            graphs.append(g)
            runs[name + "_graph"] = g.replay
            runs[name + "_eager"] = fn
        # what the calls found, once
        cases["batch_scan"]()
        cases["batch_check"]()
        cases["segments_scan"]()
        cases["segments_check"]()
        side.synchronize()
        sm1 = o1["summary"].cpu().numpy()[:32].view(A.FRAMES_CHECK_RESULT_DTYPE)[0]
        out["batch_result"] = {f: int(sm1[f]) for f in ("n_checked", "n_valid", "n_kept")}
        kept1 = o1["kept"].cpu().numpy()[:int(sm1["n_kept"])]
        chk1 = o1["check"].cpu().numpy().view(A.FRAME_CHECK_DTYPE)
        body1 = o1["body"].cpu().numpy().reshape(cap1, B1 - h - 4)
        got = [bytes(body1[r, :int(chk1[i]["length"])]) for r, i in enumerate(kept1)]
        out["batch_bodies_equal"] = got == datas
        sm2 = o2["summary"].cpu().numpy()[:S * 32].view(A.FRAMES_CHECK_RESULT_DTYPE)
        out["segments_result"] = {f: int(sm2[f].sum()) for f in ("n_checked", "n_valid", "n_kept")}
        out["segments"] = S
        times = {k: [] for k in runs}
        for rep in range(args.warmup + args.reps):
            for k, fn in runs.items():
                t = timed(fn)
                if rep >= args.warmup:
                    times[k].append(t)
        for k, v in times.items():
            out[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                              "max": round(max(v), 2)}
        for shape in ("batch", "segments"):
            out[shape + "_check_over_scan"] = round(
                out[shape + "_check_graph_us"]["median"] / out[shape + "_scan_graph_us"]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
