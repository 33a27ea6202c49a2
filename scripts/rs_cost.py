#!/usr/bin/env python3
"""Cost of demod_frames_rs_async beside the check's and the decode's launches,
in one process.

scripts/frames_decode_cost.py's method on its two shapes, without a detector:
the rows, hits, results and powers are made on the host, since the stage's
cost depends on the rows alone. Device events around each replay of a
captured graph on one stream, warm-up rounds, then medians over --reps repeats
with every figure taken once per round in turn. A 24-symbol word, a 2-byte
length, CRC-32, 2-FSK, hop 256 (R = 4), 4 194 301 windows.

  batch     1000 rows 4096 windows apart, N = 2048 symbols, n_groups = 1,
            max_frames = 2048. Plain (fec 0x100 / 0x200): B = 256, frames of 0
            .. 110 data bytes. Coded (fec 0x101 / 0x201): the decode's rows of
            Bd = 127 bytes, frames of 0 .. 50 data bytes with 4 inverted coded
            bits, which the Viterbi decoder repairs: the stage sees clean rows.
  segments  1024 groups x 8 rows, three frames each, N = 232 symbols: B = 29,
            frames of 0 .. 7 data bytes at P = 16 (n' <= 29). P = 32 does not fit
            this row, nor does any protected frame fit its decoded rows (Bd =
            13): those figures are absent.

The stage corrects its rows in place, so a replay that should meet wrong bytes
has to put them back first: each plain figure is one graph of a device copy
of the prepared rows and the stage, with clean rows and with t wrong bytes in
every codeword, and the copy alone is timed beside them.

    python scripts/rs_cost.py [--reps 30]

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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("rs_cost.py: no GPU visible (nothing is measured without one)")
    A = load_pkg()
    n, hop, freqs = 1024, 256, A.FSK2_FREQS
    cfg = A.make_cfg(freqs=freqs, n=n, hop=hop, method=A.METHOD_FFT)
    W = ((1 << 20) * n - n) // hop + 1
    R, K, L, h, kind = n // hop, 2, 24, 2, A.DEMOD_CRC32_MPEG2
    u8 = dict(dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(1)
    side = torch.cuda.Stream()
    out = {"windows": W, "hop": hop, "k": K, "phases": R, "reps": args.reps, "sync_len": L, "len_bytes": h,
           "crc": "crc32_mpeg2"}
    RES = ctypes.sizeof(A.DemodFramesResult)
    n_written_at = A.DemodFramesResult.n_written.offset

    def results(counts):
        res = np.zeros((len(counts), RES), np.uint8)
        res[:, n_written_at:n_written_at + 8] = np.array(counts, "<u8").view(np.uint8).reshape(-1, 8)
        return torch.from_numpy(res.reshape(-1)).cuda()

    def plain_rows(fec, width, lens, wrong):
        """One row a length: the protected frame, random bytes behind it, and
        `wrong` wrong bytes in every codeword (the header spared)."""
        P = A.RS_PARITY[fec & 0x300]
        rows = rng.integers(0, 256, (len(lens), width)).astype(np.uint8)
        for i, ln in enumerate(lens):
            frame = np.frombuffer(A.rs_frame_encode(rng.integers(0, 256, ln).astype(np.uint8).tobytes(), h, kind,
                                                    fec), np.uint8).copy()
            nn = h + ln + 4
            D = (len(frame) - nn) // P
            for j in range(D if wrong else 0):
                off = [o for o in list(range(j, nn, D)) + [nn + i2 * D + j for i2 in range(P)] if o >= h]
                for o in rng.choice(off, wrong, replace=False):
                    frame[o] ^= int(rng.integers(1, 256))
            rows[i, :len(frame)] = frame
        return rows

    def outputs(rows, max_len, groups):
        return dict(check=torch.empty(rows * ctypes.sizeof(A.DemodFrameCheck), **u8),
                    kept=torch.empty(rows, dtype=torch.int32, device="cuda"),
                    body=torch.empty(rows * max(max_len, 1), **u8), summary=torch.empty(32 * groups, **u8))

    with A.Demodulator(cfg) as d, torch.cuda.stream(side):
        s = side.cuda_stream
        cases, after = {}, []

        def plain_shape(tag, fec, groups, cap, N, per_group, lens_top, first_window):
            width = N // 8
            P = A.RS_PARITY[fec & 0x300]
            try:
                max_len = A.rs_max_len(width, h, kind, fec)
            except A.DemodError:
                out[tag + "_absent"] = "no protected frame fits a row of %d bytes" % width
                return
            lens_hi = min(lens_top, max_len)
            counts = [per_group] * groups
            rows_n = groups * cap
            sets = {}
            for name, wrong in (("clean", 0), ("t_errors", P // 2)):
                buf = rng.integers(0, 256, (rows_n, width)).astype(np.uint8)
                lens = rng.integers(0, lens_hi + 1, groups * per_group)
                made = plain_rows(fec, width, lens, wrong)
                idx = (np.arange(groups)[:, None] * cap + np.arange(per_group)[None, :]).reshape(-1)
                buf[idx] = made
                sets[name] = torch.from_numpy(buf.reshape(-1)).cuda()
            d_rows = torch.empty(rows_n * width, **u8)
            d_rs = torch.empty(rows_n * 16, **u8)
            d_res = results(counts)
            hits = np.zeros(rows_n, A.FRAME_HIT_DTYPE)
            hits["window"] = np.tile(first_window(np.arange(cap)), groups) if groups > 1 else first_window(np.arange(cap))
            d_hits = torch.from_numpy(hits.view(np.uint8).reshape(-1)).cuda()
            o = outputs(rows_n, max_len, groups)

            def stage():
                d.frames_rs_async(d_rows, d_res, groups, cap, N, h, kind, fec, d_rs, stream=s)
            cases[tag + "_copy"] = lambda: d_rows.copy_(sets["clean"])
            cases[tag + "_copy_stage_clean"] = lambda: (d_rows.copy_(sets["clean"]), stage())
            cases[tag + "_copy_stage_t_errors"] = lambda: (d_rows.copy_(sets["t_errors"]), stage())
            cases[tag + "_check"] = lambda: d.frames_check_coded_async(
                d_hits, d_rows, d_res, groups, cap, L, N, h, kind, o["check"], o["kept"], o["body"], o["summary"],
                fec=fec, stream=s)

            def found():
                rec = d_rs.cpu().numpy().view(A.FRAME_RS_DTYPE).reshape(groups, cap)[:, :per_group]
                sm = o["summary"].cpu().numpy().view(A.FRAMES_CHECK_RESULT_DTYPE)
                out[tag + "_result"] = {"rows": int(rec.size), "ok": int((rec["status"] == 0).sum()),
                                        "codewords": int(rec["codewords"].sum()), "corrected": int(rec["corrected"].sum()),
                                        "n_valid": int(sm["n_valid"].sum()), "row_bytes": width, "max_len": max_len}
            after.append(found)

        def coded_batch(tag, fec):
            N, cap, n_frames = 2048, 2048, 1000
            Bd = A.fec_row_bytes(N, 1, h, fec)
            max_len = A.rs_max_len(Bd, h, kind, fec)
            mag = np.ones((W, K), np.float32)
            hits = np.zeros(cap, A.FRAME_HIT_DTYPE)
            for f in range(n_frames):
                w0 = 512 + 4096 * f
                data = rng.integers(0, 256, int(rng.integers(0, min(50, max_len) + 1))).astype(np.uint8).tobytes()
                air = A.fec_frame_encode(data, h, kind, fec)
                bits = A.unpack_symbols(air, A.fec_frame_symbols(len(data), h, kind, 1, fec), 1)
                bits[rng.choice(bits.size, 4, replace=False)] ^= 1
                at = w0 + (L + np.arange(bits.size)) * R
                mag[at, bits] = 4.0
                hits["window"][f] = w0
            d_mag = torch.from_numpy(mag.reshape(-1)).cuda()
            d_hits = torch.from_numpy(hits.view(np.uint8).reshape(-1)).cuda()
            d_res = results([n_frames])
            d_rows, d_dec, d_rs = torch.empty(cap * Bd, **u8), torch.empty(cap * 16, **u8), torch.empty(cap * 16, **u8)
            work = torch.empty(A.fec_decode_workspace_size(cfg, 1, cap, N, fec), **u8)
            o = outputs(cap, max_len, 1)
            cases[tag + "_decode"] = lambda: d.frames_decode_async(d_hits, d_mag, W, None, d_res, 1, cap, L, N, h, kind,
                                                                  d_rows, d_dec, work, fec=fec, stream=s)
            cases[tag + "_stage_clean"] = lambda: d.frames_rs_async(d_rows, d_res, 1, cap, N, h, kind, fec, d_rs,
                                                                   stream=s)
            cases[tag + "_check"] = lambda: d.frames_check_coded_async(
                d_hits, d_rows, d_res, 1, cap, L, N, h, kind, o["check"], o["kept"], o["body"], o["summary"], fec=fec,
                stream=s)

            def found():
                rec = d_rs.cpu().numpy().view(A.FRAME_RS_DTYPE)[:n_frames]
                sm = o["summary"].cpu().numpy().view(A.FRAMES_CHECK_RESULT_DTYPE)
                out[tag + "_result"] = {"rows": n_frames, "ok": int((rec["status"] == 0).sum()),
                                        "corrected": int(rec["corrected"].sum()), "n_valid": int(sm["n_valid"].sum()),
                                        "row_bytes": Bd, "max_len": max_len}
            after.append(found)

        for P, flag in ((16, A.DEMOD_FEC_RS16), (32, A.DEMOD_FEC_RS32)):
            plain_shape("batch_p%d" % P, flag, 1, 2048, 2048, 1000, 110, lambda i: 512 + 4096 * i)
            plain_shape("segments_p%d" % P, flag, 1024, 8, 232, 3, 7, lambda i: 256 + 1280 * i)
            coded_batch("batch_coded_p%d" % P, flag | A.DEMOD_FEC_CONV_K7)
        runs, graphs = {}, []
        for name, fn in cases.items():      # in order: every call's inputs are left by the ones before
            fn()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn()
            graphs.append(g)
            runs[name + "_graph"] = g.replay
        for g in graphs:
            g.replay()
        side.synchronize()
        for fn in after:
            fn()

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
        for k, v in times.items():
            out[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                              "max": round(max(v), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
