#!/usr/bin/env python3
"""Cost of demod_frames_decode_async in each coded mode (include/demod.h
"punctured and interleaved"), beside fec == 1 in the same process.

scripts/frames_decode_cost.py's two shapes and its method (device events
around each replay of a captured graph of the one launch, warm-up rounds, then
medians over --reps repeats with every figure taken once per round in turn),
without the detector and the scan in front: the hits, the scan's results and
the powers are made here, as the kernel-level tests make them. 2-FSK, R = 4, a
24-symbol word, a 2-byte length and CRC-32.

  batch     1000 frames 4096 windows apart in 4 194 301 windows, rows of N =
            2048 symbols, max_frames 2048, n_groups = 1; 0 .. 50 data bytes.
  segments  1024 segments x 4096 windows with three frames each, 8 rows a
            segment; 0 .. 7 data bytes. Rows of N = 232 symbols in order and
            of N = 256 interleaved (a row must hold a whole block).

Every mode decodes the same data bytes, so T(len), the steps a row runs, is the
same in every mode; what differs is where a step's soft values sit on the air.
Each frame carries 4 inverted air bits; the decoded rows are compared with the
frames sent. The figure per mode is also given per trellis step (median /
mean steps a row) relative to fec == 1.

    python scripts/fec_modes_cost.py [--reps 30]

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
MODES = (0x01, 0x11, 0x21, 0x41, 0x51, 0x61)


def load_pkg():
    spec = importlib.util.spec_from_file_location(
        "audio_network_amd", os.path.join(ROOT, "audio-network_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["audio_network_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("fec_modes_cost.py: no GPU visible (nothing is measured without one)")
    A = load_pkg()
    n, hop, freqs = 1024, 256, A.FSK2_FREQS
    cfg = A.make_cfg(freqs=freqs, n=n, hop=hop, method=A.METHOD_FFT)
    W = ((1 << 20) * n - n) // hop + 1
    R, K, L, h, kind = n // hop, 2, 24, 2, A.DEMOD_CRC32_MPEG2
    u8 = dict(dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(1)
    base_P = rng.integers(1, 300, (W, K)).astype(np.float32)
    res_bytes, n_hits_at = ctypes.sizeof(A.DemodFramesResult), 528
    hit_dtype = np.dtype([("window", "<u8"), ("errors", "<u4"), ("reserved", "<u4")])
    assert hit_dtype.itemsize == ctypes.sizeof(A.DemodFrameHit)

    def results(counts):
        res = np.zeros((len(counts), res_bytes), np.uint8)
        raw = np.array(counts, "<u8").view(np.uint8).reshape(-1, 8)
        res[:, n_hits_at:n_hits_at + 8] = raw
        res[:, n_hits_at + 8:n_hits_at + 16] = raw
        return torch.from_numpy(res.reshape(-1)).cuda()

    def plant(P, w0, data, fec):
        """The frame's symbols behind a word at w0: the decided tone 1000 .. 1999."""
        air = np.unpackbits(np.frombuffer(A.fec_frame_encode(data, h, kind, fec), np.uint8))
        air = air[:A.fec_frame_symbols(len(data), h, kind, 1, fec)].copy()
        air[rng.choice(air.size, 4, replace=False)] ^= 1
        at = w0 + (L + np.arange(air.size)) * R
        P[at, air] = rng.integers(1000, 2000, air.size)

    # batch
    n_frames, N1, cap1 = 1000, 2048, 2048
    datas1 = [rng.integers(0, 256, int(rng.integers(0, 51))).astype(np.uint8).tobytes() for _ in range(n_frames)]
    hits1 = np.zeros(cap1, hit_dtype)
    hits1["window"][:n_frames] = 1 + 512 + 4096 * np.arange(n_frames)
    # segments
    S, cap2 = 1024, 8
    first = np.arange(S, dtype=np.int64) * 4096
    datas2 = [rng.integers(0, 256, int(rng.integers(0, 8))).astype(np.uint8).tobytes() for _ in range(3 * S)]
    hits2 = np.zeros((S, cap2), hit_dtype)
    hits2["window"][:, :3] = 1 + 256 + 1280 * np.arange(3)[None, :]           # relative to first[g]
    out = {"windows": W, "hop": hop, "k": K, "phases": R, "reps": args.reps, "sync_len": L, "len_bytes": h,
           "crc": "crc32_mpeg2", "modes": {}}
    runs, keep = {}, []
    side = torch.cuda.Stream()
    with A.Demodulator(cfg) as d, torch.cuda.stream(side):
        s = side.cuda_stream
        d_hits1, d_res1 = torch.from_numpy(hits1.view(np.uint8)).cuda(), results([n_frames])
        d_hits2, d_res2 = torch.from_numpy(hits2.view(np.uint8).reshape(-1)).cuda(), results([3] * S)
        d_first = torch.from_numpy(first).cuda()
        for fec in MODES:
            N2 = 256 if fec & A.DEMOD_FEC_INTERLEAVE else 232
            P1, P2 = base_P.copy(), base_P.copy()
            for f, data in enumerate(datas1):
                plant(P1, int(hits1["window"][f]), data, fec)
            for g in range(S):
                for f in range(3):
                    plant(P2, int(first[g]) + int(hits2["window"][g, f]), datas2[3 * g + f], fec)
            info = {}
            for tag, P, d_hits, d_res, d_f, groups, cap, N, datas in (
                    ("batch", P1, d_hits1, d_res1, None, 1, cap1, N1, datas1),
                    ("segments", P2, d_hits2, d_res2, d_first, S, cap2, N2, datas2)):
                Bd = A.fec_row_bytes(N, 1, h, fec)
                d_P = torch.from_numpy(P.reshape(-1)).cuda()
                rows, dec = torch.zeros(groups * cap * Bd, **u8), torch.zeros(groups * cap * 16, **u8)
                work = torch.empty(A.fec_decode_workspace_size(cfg, groups, cap, N, fec), **u8)

                def fn(d_hits=d_hits, d_P=d_P, d_f=d_f, d_res=d_res, groups=groups, cap=cap, N=N, rows=rows,
                       dec=dec, work=work, fec=fec):
                    d.frames_decode_async(d_hits, d_P, W, d_f, d_res, groups, cap, L, N, h, kind, rows, dec, work,
                                          fec=fec, stream=s)
                fn()
                side.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    fn()
                keep.append((g, d_P, rows, dec, work))
                runs[(fec, tag)] = g.replay
                per = len(datas) // groups
                got_rows = rows.cpu().numpy().reshape(groups, cap, Bd)[:, :per].reshape(len(datas), Bd)
                dd = dec.cpu().numpy().view(A.FRAME_DECODE_DTYPE).reshape(groups, cap)[:, :per].reshape(-1)
                frames = [A.checked_frame_encode(data, h, kind) for data in datas]
                info[tag] = {"frame_symbols": N, "row_bytes": Bd, "workspace_bytes": int(work.numel()),
                             "rows": len(datas), "ok": int((dd["status"] == 0).sum()),
                             "rows_equal": sum(bytes(r[:len(f)]) == f for r, f in zip(got_rows, frames)),
                             "mean_steps": round(float(dd["steps"].mean()), 1), "max_steps": int(dd["steps"].max())}
            out["modes"][hex(fec)] = info

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(side)
            fn()
            b.record(side)
            b.synchronize()
            return a.elapsed_time(b) * 1e3     # us

        times = {k: [] for k in runs}
        for rep in range(args.warmup + args.reps):
            for k, fn in runs.items():
                t = timed(fn)
                if rep >= args.warmup:
                    times[k].append(t)
    for (fec, tag), v in times.items():
        out["modes"][hex(fec)][tag]["decode_graph_us"] = {
            "median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    for tag in ("batch", "segments"):
        one = out["modes"]["0x1"][tag]
        for fec in MODES:
            m = out["modes"][hex(fec)][tag]
            m["over_fec1"] = round(m["decode_graph_us"]["median"] / one["decode_graph_us"]["median"], 3)
            m["per_step_over_fec1"] = round((m["decode_graph_us"]["median"] / m["mean_steps"]) /
                                            (one["decode_graph_us"]["median"] / one["mean_steps"]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
