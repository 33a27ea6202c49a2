#!/usr/bin/env python3
"""Cost of erasure decoding's two launches beside demod_frames_rs_async, in one
process.

scripts/rs_cost.py's method on its two plain shapes: rows, masks, hits, results
and powers are made on the host; device events around each replay of a captured
graph on one stream, warm-up rounds, then medians over --reps repeats with
every figure taken once per round in turn. A 24-symbol word, a 2-byte length,
CRC-32, 2-FSK, hop 256 (R = 4), 4 194 301 windows.

  batch     1000 rows 4096 windows apart, N = 2048 symbols, n_groups = 1,
            max_frames = 2048, B = 256 (Wm = 4), frames of 0 .. 110 data bytes.
  segments  1024 groups x 8 rows, three frames each, N = 232 symbols: B = 29
            (Wm = 1), frames of 0 .. 7 data bytes at P = 16; P = 32 does not fit.

The stages correct their rows in place, so each figure is one graph of a device
copy of the prepared rows and the stage, and the copy alone is timed beside
them:

  plain_clean, plain_t_errors      demod_frames_rs_async, as scripts/rs_cost.py
  erase_zero_mask                  the erasure stage, clean rows, an all-zero mask
  erase_t_errors                   the erasure stage, t unflagged wrong bytes a
                                   codeword, an all-zero mask
  erase_p_flagged                  the erasure stage, P flagged wrong bytes a
                                   codeword
  producer                         demod_frames_erasures_async alone, level 16

    python scripts/rs_erasures_cost.py [--reps 30]

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
        sys.exit("rs_erasures_cost.py: no GPU visible (nothing is measured without one)")
    A = load_pkg()
    n, hop, freqs = 1024, 256, A.FSK2_FREQS
    cfg = A.make_cfg(freqs=freqs, n=n, hop=hop, method=A.METHOD_FFT)
    W = ((1 << 20) * n - n) // hop + 1
    R, K, L, h, kind = n // hop, 2, 24, 2, A.DEMOD_CRC32_MPEG2
    u8 = dict(dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(1)
    side = torch.cuda.Stream()
    out = {"windows": W, "hop": hop, "k": K, "phases": R, "reps": args.reps, "sync_len": L, "len_bytes": h,
           "crc": "crc32_mpeg2", "level": 16}
    RES = ctypes.sizeof(A.DemodFramesResult)
    n_written_at = A.DemodFramesResult.n_written.offset

    def results(counts):
        res = np.zeros((len(counts), RES), np.uint8)
        res[:, n_written_at:n_written_at + 8] = np.array(counts, "<u8").view(np.uint8).reshape(-1, 8)
        return torch.from_numpy(res.reshape(-1)).cuda()

    def plain_rows(fec, width, lens, wrong, flagged):
        """One row a length: the protected frame, random bytes behind it, `wrong`
        wrong bytes in every codeword (the header spared), flagged or not."""
        P = A.RS_PARITY[fec & 0x300]
        rows = rng.integers(0, 256, (len(lens), width)).astype(np.uint8)
        masks = np.zeros((len(lens), A.mask_words(width)), np.uint64)
        for i, ln in enumerate(lens):
            frame = np.frombuffer(A.rs_frame_encode(rng.integers(0, 256, ln).astype(np.uint8).tobytes(), h, kind,
                                                    fec), np.uint8).copy()
            nn = h + ln + 4
            D = (len(frame) - nn) // P
            flags = np.zeros(width, bool)
            for j in range(D if wrong else 0):
                off = [o for o in list(range(j, nn, D)) + [nn + i2 * D + j for i2 in range(P)] if o >= h]
                for o in rng.choice(off, wrong, replace=False):
                    frame[o] ^= int(rng.integers(1, 256))
                    flags[o] = flagged
            rows[i, :len(frame)] = frame
            masks[i] = A.pack_mask(flags, width)
        return rows, masks

    with A.Demodulator(cfg) as d, torch.cuda.stream(side):
        s = side.cuda_stream
        cases, after = {}, []
        d_mag = torch.from_numpy(rng.random(W * K, dtype=np.float32)).cuda()

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
            rows_n, Wm = groups * cap, A.mask_words(width)
            idx = (np.arange(groups)[:, None] * cap + np.arange(per_group)[None, :]).reshape(-1)
            sets = {}
            for name, wrong, flagged in (("clean", 0, False), ("t_errors", P // 2, False), ("p_flagged", P, True)):
                buf = rng.integers(0, 256, (rows_n, width)).astype(np.uint8)
                msk = np.zeros((rows_n, Wm), np.uint64)
                lens = rng.integers(0, lens_hi + 1, groups * per_group)
                buf[idx], msk[idx] = plain_rows(fec, width, lens, wrong, flagged)
                sets[name] = (torch.from_numpy(buf.reshape(-1)).cuda(),
                              torch.from_numpy(msk.view(np.int64).reshape(-1)).cuda())
            d_rows = torch.empty(rows_n * width, **u8)
            d_rs, d_erec = torch.empty(rows_n * 16, **u8), torch.empty(rows_n * 16, **u8)
            d_made = torch.empty(rows_n * Wm, dtype=torch.int64, device="cuda")
            d_res = results(counts)
            hits = np.zeros(rows_n, A.FRAME_HIT_DTYPE)
            hits["window"] = np.tile(first_window(np.arange(cap)), groups) if groups > 1 else first_window(np.arange(cap))
            d_hits = torch.from_numpy(hits.view(np.uint8).reshape(-1)).cuda()

            def plain():
                d.frames_rs_async(d_rows, d_res, groups, cap, N, h, kind, fec, d_rs, stream=s)

            def erase(name):
                d.frames_rs_erasures_async(d_rows, sets[name][1], d_res, groups, cap, N, h, kind, fec, d_rs, d_erec,
                                           stream=s)
            cases[tag + "_copy"] = lambda: d_rows.copy_(sets["clean"][0])
            cases[tag + "_copy_plain_clean"] = lambda: (d_rows.copy_(sets["clean"][0]), plain())
            cases[tag + "_copy_plain_t_errors"] = lambda: (d_rows.copy_(sets["t_errors"][0]), plain())
            cases[tag + "_copy_erase_zero_mask"] = lambda: (d_rows.copy_(sets["clean"][0]), erase("clean"))
            cases[tag + "_copy_erase_t_errors"] = lambda: (d_rows.copy_(sets["t_errors"][0]), erase("t_errors"))
            cases[tag + "_copy_erase_p_flagged"] = lambda: (d_rows.copy_(sets["p_flagged"][0]), erase("p_flagged"))
            cases[tag + "_producer"] = lambda: d.frames_erasures_async(d_hits, d_mag, W, None, d_res, groups, cap, L, N,
                                                                      16, d_made, stream=s)

            def found():   # after the graphs' first replays: the last stage to run was p_flagged's
                rec = d_rs.cpu().numpy().view(A.FRAME_RS_DTYPE).reshape(groups, cap)[:, :per_group]
                er = d_erec.cpu().numpy().view(A.FRAME_ERASE_DTYPE).reshape(groups, cap)[:, :per_group]
                made = d_made.cpu().numpy().view(np.uint64).reshape(groups, cap, Wm)[:, :per_group]
                out[tag + "_result"] = {"rows": int(rec.size), "ok": int((rec["status"] == 0).sum()),
                                        "codewords": int(rec["codewords"].sum()), "corrected": int(rec["corrected"].sum()),
                                        "erased": int(er["erased"].sum()), "used": int(er["used"].sum()),
                                        "fallback": int(er["fallback"].sum()),
                                        "produced_flags": int(sum(bin(int(w)).count("1") for w in made.reshape(-1))),
                                        "row_bytes": width, "mask_words": Wm, "max_len": max_len}
            after.append(found)

        for P, flag in ((16, A.DEMOD_FEC_RS16), (32, A.DEMOD_FEC_RS32)):
            plain_shape("batch_p%d" % P, flag, 1, 2048, 2048, 1000, 110, lambda i: 512 + 4096 * i)
            plain_shape("segments_p%d" % P, flag, 1024, 8, 232, 3, 7, lambda i: 256 + 1280 * i)
        runs, graphs = {}, []
        for name, fn in cases.items():
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
