#!/usr/bin/env python3
"""Cost of demod_frames_decode_async and demod_frames_check_coded_async beside
the frame scan and demod_frames_check_async, in one process.

scripts/frames_check_cost.py's method and its two shapes: configs[3] (the
sliding 1024-point FFT detector, hop 256, 2-FSK, 2^20 x 1024 synthetic samples
= 4 194 301 windows), device events around each replay on one stream, warm-up
rounds, then medians over --reps repeats with every figure taken once per
round in turn. Each call is timed as one replay of a captured graph of its
launches. A 24-symbol word, a 2-byte length and CRC-32.

  batch     1000 frames 4096 windows apart, rows of N = 2048 symbols, n_groups
            = 1. Plain: checked frames of 0 .. 110 data bytes (B = 256),
            demod_frames_async with packed rows and demod_frames_check_async,
            as frames_check_cost.py times them. Coded: frames of 0 .. 50 data
            bytes (St = 1024 steps a row at most, Bd = 127, max_len = 121; a
            row's forward pass stops at T(len) <= 454), the scan without rows,
            demod_frames_decode_async and demod_frames_check_coded_async.
  segments  1024 segments x 4096 windows with three frames each, rows of N =
            232 symbols, 8 rows a segment, n_groups = 1024. Plain: 0 .. 23 data
            bytes (B = 29). Coded: 0 .. 7 data bytes (St = 116, Bd = 13,
            max_len = 7).

The coded frames are planted in copies of the detector's symbols and powers
(the decided tone 4 x the other at a frame's windows), with 4 inverted coded
bits a frame.

    python scripts/frames_decode_cost.py [--windows 1048576] [--reps 30]

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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("frames_decode_cost.py: no GPU visible (nothing is measured without one)")
    A = load_pkg()
    n, hop, freqs = 1024, 256, A.FSK2_FREQS
    gen_cfg = A.make_cfg(freqs=freqs, n=n)
    cfg = A.make_cfg(freqs=freqs, n=n, hop=hop, method=A.METHOD_FFT)
    Wg = args.windows
    W = (Wg * n - n) // hop + 1
    R, K, L, h, kind, fec = n // hop, len(freqs), 24, 2, A.DEMOD_CRC32_MPEG2, A.DEMOD_FEC_CONV_K7
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_pcm = torch.empty((Wg, n), dtype=torch.int16, device="cuda")
    A.synth_fsk(gen_cfg, A.BENCH_SEED, Wg, 8000, 400, d_pcm, None)
    d_sym = torch.empty(W, **u8)
    d_mag = torch.empty((W, K), dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(1)
    word = rng.integers(0, K, L).astype(np.uint8)
    side = torch.cuda.Stream()
    out = {"windows": W, "hop": hop, "k": K, "phases": R, "method": "fft", "reps": args.reps, "sync_len": L,
           "len_bytes": h, "crc": "crc32_mpeg2", "fec": "conv_k7"}

    def plain_symbols(data):
        frame = A.checked_frame_encode(data, h, kind)
        return A.unpack_symbols(frame, len(frame) * 8, 1)

    def coded_symbols(data):
        coded = A.coded_frame_encode(data, h, kind)
        sym = A.unpack_symbols(coded, 2 * A.coded_frame_steps(len(data), h, kind), 1)
        sym[rng.choice(sym.size, 4, replace=False)] ^= 1
        return sym

    def outputs(rows, width):
        max_len = width - h - 4
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
        base, mags = d_sym.cpu().numpy(), d_mag.cpu().numpy()

        def plant(sym, mag, w0, seq):
            at = w0 + np.arange(len(seq)) * R
            sym[at] = seq
            if mag is not None:                      # the decided tone 4 x the other: the phase metric keeps its order
                top = mag[at].max(axis=1)
                mag[at] = (top / 4)[:, None]
                mag[at, seq] = top

        # batch: 1000 frames 4096 windows apart, rows of 2048 symbols
        n_frames = min(1000, (W - 16384) // 4096)
        N1, cap1 = 2048, 2048
        B1, Bd1 = N1 // 8, A.coded_row_bytes(N1, 1, h)
        sym1, sym1c, mag1c = base.copy(), base.copy(), mags.copy()
        datas1 = [rng.integers(0, 256, int(rng.integers(0, 51))).astype(np.uint8).tobytes() for _ in range(n_frames)]
        for f in range(n_frames):
            w0 = phase + 4096 * f + 512
            plant(sym1, None, w0, np.concatenate([word, plain_symbols(
                rng.integers(0, 256, int(rng.integers(0, 111))).astype(np.uint8).tobytes())]))
            plant(sym1c, mag1c, w0, np.concatenate([word, coded_symbols(datas1[f])]))
        d_sym1, d_sym1c, d_mag1c = (torch.from_numpy(a).cuda() for a in (sym1, sym1c, mag1c))
        hits1, packed1 = torch.empty(cap1 * 16, **u8), torch.empty(cap1 * B1, **u8)
        hits1c, res1c = torch.empty(cap1 * 16, **u8), torch.empty_like(d_res)
        rows1 = torch.empty(cap1 * Bd1, **u8)
        dec1 = torch.empty(cap1 * 16, **u8)
        fwork1 = torch.empty(A.frames_decode_workspace_size(cfg, 1, cap1, N1), **u8)
        o1, o1c = outputs(cap1, B1), outputs(cap1, Bd1)

        # segments: 1024 x 4096 windows, three frames each, rows of 232 symbols
        S, N2, cap2 = min(1024, -(-W // 4096)), 232, 8
        B2, Bd2 = N2 // 8, A.coded_row_bytes(N2, 1, h)
        first = np.arange(S, dtype=np.int64) * 4096
        count = np.minimum(4096, W - first).astype(np.int32)
        sym2, sym2c, mag2c = base.copy(), base.copy(), mags.copy()
        datas2 = []
        for g in range(S):
            for f in range(3):
                w0 = int(first[g]) + phase + 256 + 1280 * f
                if w0 + (L + N2) * R >= W:
                    continue
                plant(sym2, None, w0, np.concatenate([word, plain_symbols(
                    rng.integers(0, 256, int(rng.integers(0, 24))).astype(np.uint8).tobytes())]))
                datas2.append(rng.integers(0, 256, int(rng.integers(0, 8))).astype(np.uint8).tobytes())
                plant(sym2c, mag2c, w0, np.concatenate([word, coded_symbols(datas2[-1])]))
        d_sym2, d_sym2c, d_mag2c = (torch.from_numpy(a).cuda() for a in (sym2, sym2c, mag2c))
        d_first, d_count = torch.from_numpy(first).cuda(), torch.from_numpy(count).cuda()
        hits2, packed2 = torch.empty(S * cap2 * 16, **u8), torch.empty(S * cap2 * B2, **u8)
        d_res2 = torch.empty(S * ctypes.sizeof(A.DemodFramesResult), **u8)
        hits2c, res2c = torch.empty_like(hits2), torch.empty_like(d_res2)
        d_work2 = torch.empty(A.frames_segments_workspace_size(cfg, S, W), **u8)
        rows2, dec2 = torch.empty(S * cap2 * Bd2, **u8), torch.empty(S * cap2 * 16, **u8)
        fwork2 = torch.empty(A.frames_decode_workspace_size(cfg, S, cap2, N2), **u8)
        o2, o2c = outputs(S * cap2, B2), outputs(S * cap2, Bd2)
        out["decode_workspace_bytes"] = {"batch": int(fwork1.numel()), "segments": int(fwork2.numel())}

        cases = {
            "batch_scan": lambda: d.frames_async(d_sym1, d_mag, W, word, 0, N1, hits1, None, packed1, cap1, d_res,
                                                 d_work, stream=s),
            "batch_check": lambda: d.frames_check_async(hits1, packed1, d_res, 1, cap1, L, N1, h, kind, o1["check"],
                                                        o1["kept"], o1["body"], o1["summary"], stream=s),
            "batch_scan_no_rows": lambda: d.frames_async(d_sym1c, d_mag1c, W, word, 0, N1, hits1c, None, None, cap1,
                                                         res1c, d_work, stream=s),
            "batch_decode": lambda: d.frames_decode_async(hits1c, d_mag1c.view(-1), W, None, res1c, 1, cap1, L, N1, h,
                                                          kind, rows1, dec1, fwork1, fec=fec, stream=s),
            "batch_check_coded": lambda: d.frames_check_coded_async(hits1c, rows1, res1c, 1, cap1, L, N1, h, kind,
                                                                    o1c["check"], o1c["kept"], o1c["body"],
                                                                    o1c["summary"], fec=fec, stream=s),
            "segments_scan": lambda: d.frames_segments_async(d_sym2, d_mag, W, d_first, d_count, S, word, 0, N2,
                                                             hits2, None, packed2, cap2, d_res2, d_work2, stream=s),
            "segments_check": lambda: d.frames_check_async(hits2, packed2, d_res2, S, cap2, L, N2, h, kind,
                                                           o2["check"], o2["kept"], o2["body"], o2["summary"],
                                                           stream=s),
            "segments_scan_no_rows": lambda: d.frames_segments_async(d_sym2c, d_mag2c, W, d_first, d_count, S, word,
                                                                     0, N2, hits2c, None, None, cap2, res2c, d_work2,
                                                                     stream=s),
            "segments_decode": lambda: d.frames_decode_async(hits2c, d_mag2c.view(-1), W, d_first, res2c, S, cap2, L,
                                                             N2, h, kind, rows2, dec2, fwork2, fec=fec, stream=s),
            "segments_check_coded": lambda: d.frames_check_coded_async(hits2c, rows2, res2c, S, cap2, L, N2, h, kind,
                                                                       o2c["check"], o2c["kept"], o2c["body"],
                                                                       o2c["summary"], fec=fec, stream=s),
        }
        runs = {}
        graphs = []
        for name, fn in cases.items():      # in order: every call's inputs are left by the ones before
            fn()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn()
            graphs.append(g)
            runs[name + "_graph"] = g.replay
        for fn in cases.values():
            fn()
        side.synchronize()
        # what the calls found, once
        for tag, o, oc, dec, rows, width, cap, datas, groups in (
                ("batch", o1, o1c, dec1, rows1, Bd1, cap1, datas1, 1),
                ("segments", o2, o2c, dec2, rows2, Bd2, cap2, datas2, S)):
            sm = o["summary"].cpu().numpy()[:groups * 32].view(A.FRAMES_CHECK_RESULT_DTYPE)
            smc = oc["summary"].cpu().numpy()[:groups * 32].view(A.FRAMES_CHECK_RESULT_DTYPE)
            out[tag + "_result"] = {f: int(sm[f].sum()) for f in ("n_checked", "n_valid", "n_kept")}
            out[tag + "_coded_result"] = {f: int(smc[f].sum()) for f in ("n_checked", "n_valid", "n_kept")}
            chk = oc["check"].cpu().numpy().view(A.FRAME_CHECK_DTYPE).reshape(groups, cap)
            kept = oc["kept"].cpu().numpy().reshape(groups, cap)
            body = oc["body"].cpu().numpy().reshape(groups, cap, width - h - 4)
            got = [bytes(body[g, r, :int(chk[g, kept[g, r]]["length"])])
                   for g in range(groups) for r in range(int(smc[g]["n_kept"]))]
            out[tag + "_coded_bodies_equal"] = got == datas
            dd = dec.cpu().numpy().view(A.FRAME_DECODE_DTYPE).reshape(groups, cap)
            live = np.concatenate([dd[g, :int(smc[g]["n_checked"])] for g in range(groups)])
            out[tag + "_decode_steps"] = {"rows": int(live.size), "ok": int((live["status"] == 0).sum()),
                                          "mean": round(float(live["steps"].mean()), 1) if live.size else 0.0,
                                          "max": int(live["steps"].max()) if live.size else 0}
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
            scan = out[shape + "_scan_graph_us"]["median"]
            out[shape + "_decode_over_scan"] = round(out[shape + "_decode_graph_us"]["median"] / scan, 3)
            out[shape + "_check_coded_over_check"] = round(
                out[shape + "_check_coded_graph_us"]["median"] / out[shape + "_check_graph_us"]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
