#!/usr/bin/env python3
"""bench.py — Goertzel FSK demodulation throughput on MI355X.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1
launched by torch.distributed.run, one rank per GPU. Called with --gpus N > 1
and no WORLD_SIZE in the environment, bench.py starts torch.distributed.run
itself (as a child process, before any GPU call) and relays its output; a
WORLD_SIZE different from --gpus is an error. Rank 0 prints ONE JSON line.

Headline workload (BASELINE.json configs[1]): 2-FSK Goertzel on 2^20 windows
x 1024 int16 samples (2 GiB) per GPU, resident in HBM before timing. One step
= one demod_batch_async over the whole batch (the detector launch(es), symbols
+ |X_k|^2 written to HBM, and the decision rescue's launch)
and, for N > 1, the RCCL all-gather of every rank's decoded symbols (the only
collective of the path). Weak scaling: every rank demodulates
its own 2^20 windows (disjoint slices of one seeded stream).

value = samples demodulated by all ranks / wall time per step (Msamples/s).
roofline = algorithmic bytes per launch (2048 B in + 1 B symbol + 4K B
magnitudes per window) / mean batch duration from HIP events
recorded on the launch stream, vs the 8 TB/s HBM peak. traffic = HBM bytes per
launch from the committed rocprofv3 PMC summary (profiles/), or null.

A plain run (`--gpus N --steps K --warmup W`) does what that figure needs and
no more: set up, warm up, time the K steps, write the outputs if
--dump-outputs DIR is given (the last timed step's symbols and magnitudes as
DIR/<name>.npy, float32, at most 64 MB), print the line. Everything below
(cpu_baseline, parity_all, parity_sample, rescue, sustained and the extra
entries) is measured only with --full.

cpu_baseline = the oracle's C restatement (OpenMP over the host cores this
process may use) on a bounded sample of the same windows (rank 0, N = 1 only),
median of >= 5 timed repetitions; its output doubles as a parity check of the
timed GPU output on that sample (parity_sample, with the top-2 decision-margin
histogram SURVEY §7 asks for, at sigma 400 and at the sigma 2000 stress level).
rescue = the same step with the decision rescue switched off
(FSKD_NO_RESCUE=1), i.e. the rescue's cost.

Extra entries of a --full run:
  * N = 1: configs[2] (8-FSK) "fsk8"; configs[3] (sliding FFT, hop 256)
    "fft_hop256" with an oracle parity sample of 16384 consecutive windows, and
    with the full 513-bin spectrum stored, "fft_hop256_spectrum"; configs[4]
    "streams" (1024 streams, RCCL at world size 1, one HIP graph per step; a
    child `bench.py --config streams --force-dist`); "host_e2e", the
    PCIe-inclusive rate of a 2 GiB host-buffer demod_batch against the raw
    host-to-device copy rate;
  * N > 1: configs[4] "streams" sharded over the N ranks (strong scaling,
    graph step, RCCL frame gather), with scaling_vs_n1 against the same
    workload on rank 0's GPU alone in the same job.

Defaults: 200 timed steps after 20 warmup steps (the warmup is at least 64
launches, MIN_WARMUP), so each config keeps the GPU busy for 0.1-0.5 s
rather than a few ms. "sustained" (N = 1 headline, --full --sustain 6): the same
step back to back for ~6 s, the steady rate over seconds, during which an
outside utilisation sampler sees the GPU busy.
"""
import argparse
import importlib.util
import json
import math
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
VALU_PEAK_TFLOPS = 157.3  # MI355X fp32 vector peak (MI355X_MICROARCH.md)
METRIC = "PCM Msamples/s demodulated + symbol-error-rate vs reference, 1/2/4/8 MI355X"
MIN_WARMUP = 64
# HIP event pairs on every EV_EVERY-th timed step only: a pair on every step
# adds an ~8 us bubble per 0.3 ms step (scripts/step_gap_probe.py: 310.9 vs
# 302.8 us per step), which ms_per_step would carry
EV_EVERY = 4
MARGIN_BAND = 4e-5  # 4 x the 1e-5 magnitude bar: decisions closer than this are fp32-ill-posed


def load_pkg():
    spec = importlib.util.spec_from_file_location(
        "audio_network_amd", os.path.join(ROOT, "audio-network_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["audio_network_amd"] = mod
    spec.loader.exec_module(mod)
    spec = importlib.util.spec_from_file_location(
        "audio_network_amd.dist", os.path.join(ROOT, "audio-network_amd", "dist.py"))
    dmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dmod)
    return mod, dmod


def pmc_traffic(config: str, windows: int, hop: int = 1024):
    """HBM bytes per launch from profiles/pmc_<config>.json (rocprofv3 PMC)."""
    path = os.path.join(ROOT, "profiles", f"pmc_{config}.json")
    if not os.path.exists(path):
        return None
    try:
        d = json.load(open(path))
        if int(d.get("windows", -1)) != windows or int(d.get("hop", 1024)) != hop:
            return None
        return float(d["hbm_bytes_per_launch"])
    except Exception:
        return None


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_share():
    """(cpus this process may run on, cgroup CPU quota in cores or None,
    threads to use, why). The GPU box hands each GPU a share of the host:
    os.cpu_count() shows the whole machine, sched_getaffinity and the cgroup
    quota show what this process can actually use."""
    visible = os.cpu_count() or 1
    try:
        affinity = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        affinity = visible
    quota = None
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(p)
    except (OSError, ValueError):
        pass
    threads = affinity
    why = "all cpus in this process's affinity mask"
    if quota is not None and math.ceil(quota) < threads:
        threads = max(1, math.ceil(quota))
        why = f"cgroup cpu.max quota of {quota:g} cores (more threads would only be throttled)"
    return visible, affinity, quota, threads, why


def margin_stats(P: np.ndarray) -> dict:
    """Top-2 decision margin (P1 - P2) / P1 per window: min, count inside the
    fp32-ill-posed band, and a log-binned histogram."""
    if P.shape[1] < 2 or not len(P):
        return {}
    Ps = np.sort(P, axis=1)
    m = (Ps[:, -1] - Ps[:, -2]) / np.maximum(Ps[:, -1], 1e-300)
    edges = [0.0, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0 + 1e-12]
    hist, _ = np.histogram(m, bins=edges)
    return {"windows": int(m.size), "min_margin": float(m.min()),
            "below_4e-5": int((m < MARGIN_BAND).sum()),
            "hist_edges": ["0", "1e-6", "1e-5", "1e-4", "1e-3", "1e-2", "1e-1", "1"],
            "hist_counts": [int(c) for c in hist]}


def cpu_baseline(d_pcm, d_sym, d_mag, freqs, seconds: float, threads: int, fft: bool, hop: int,
                 reps: int = 7):
    """Oracle (C, OpenMP) on a bounded sample of the timed windows: the first
    S stream windows (Goertzel) or the FFT windows over the first S*n samples.
    Rate = median over `reps` repetitions of ~seconds/reps each."""
    sys.path.insert(0, ROOT)
    from oracle import oracle as O

    n = 1024
    S = min(d_pcm.shape[0], 4096 if fft else 65536)
    flat = d_pcm[:S].cpu().numpy().reshape(-1)
    n_win = (S * n - n) // hop + 1
    gsym = d_sym[:n_win].cpu().numpy()
    gmag = d_mag[:n_win].cpu().numpy().astype(np.float64) if d_mag is not None else None

    def run(x, th):
        if fft:
            return O.fft_demod(x, freqs, n, hop, threads=th)
        return O.goertzel(x, freqs, n, hop, threads=th)

    def rep_rates(fn, samples, budget, nrep):
        rates = []
        for _ in range(nrep):
            passes, t0 = 0, time.perf_counter()
            while True:
                fn()
                passes += 1
                el = time.perf_counter() - t0
                if el >= budget:
                    break
            rates.append(passes * samples / el / 1e6)
        return rates

    sym, P = run(flat, threads)  # warm + parity reference
    rates = rep_rates(lambda: run(flat, threads), S * n, seconds / reps, reps)
    # single-thread double and fp32 rates on a slice of the same sample
    S1 = max(1, S // 16)
    flat1 = flat[:S1 * n]
    r1 = rep_rates(lambda: run(flat1, 1), S1 * n, max(0.2, seconds / 25), 5)
    r1f = None
    if not fft and hop == n:
        r1f = rep_rates(lambda: O.goertzel_f32(flat1, freqs, n), S1 * n, max(0.2, seconds / 25), 5)
    parity = {"windows_checked": int(n_win), "symbol_mismatches": int((sym != gsym).sum())}
    if gmag is not None:
        parity["max_rel_mag_err"] = float((np.abs(gmag - P).max(1) / P.max(1)).max())
    parity["margin"] = margin_stats(P)
    what = ("double radix-2 FFT, argmax over tone bins" if fft else "double Goertzel")
    med = float(np.median(rates))
    base = {"value": round(med, 3), "unit": "Msamples/s", "cores": int(threads),
            "kind": "port", "reps": len(rates),
            "rep_values": [round(r, 1) for r in rates],
            "single_thread_value": round(float(np.median(r1)), 3),
            "single_thread_fp32_value": round(float(np.median(r1f)), 3) if r1f else None,
            "host_cpu": cpu_model(),
            "sample": f"first {S * n} samples ({n_win} windows, hop {hop}) of the timed batch, "
                      f"median of {len(rates)} reps of {seconds / reps:.1f} s, "
                      f"oracle/fsk_oracle.c {what}, OpenMP {threads} threads"}
    return base, parity


def stress_parity(A, O, cfg, freqs, sigma: int, W: int, dev, torch, threads: int):
    """GPU vs oracle on a fresh W-window sample at noise sigma (the σ = 2000
    stress level of SURVEY §8d): symbol mismatches, magnitude error, margins."""
    d_pcm = torch.empty((W, 1024), dtype=torch.int16, device=dev)
    d_true = torch.empty(W, dtype=torch.uint8, device=dev)
    d_sym = torch.empty(W, dtype=torch.uint8, device=dev)
    d_mag = torch.empty((W, len(freqs)), dtype=torch.float32, device=dev)
    A.synth_fsk(cfg, A.BENCH_SEED ^ sigma, W, 8000, sigma, d_pcm, d_true)
    with A.Demodulator(cfg) as d:
        d.batch_device(d_pcm, W, d_sym, d_mag)
    sym, P = O.goertzel(d_pcm.cpu().numpy(), freqs, 1024, threads=threads)
    gs, gm = d_sym.cpu().numpy(), d_mag.cpu().numpy().astype(np.float64)
    out = {"sigma": sigma, "windows_checked": W, "symbol_mismatches": int((gs != sym).sum()),
           "transmitted_symbol_errors": int((gs != d_true.cpu().numpy()).sum()),
           "max_rel_mag_err": float((np.abs(gm - P).max(1) / P.max(1)).max()),
           "margin": margin_stats(P)}
    return out


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def hip_runtime():
    """The process's HIP runtime (torch's libamdhip64.so.7, which
    libfskdemod.so binds too: one runtime per process)."""
    import ctypes
    h = ctypes.CDLL("libamdhip64.so.7")
    for f in ("hipGetLastError", "hipMalloc", "hipStreamCreateWithFlags"):
        getattr(h, f).restype = ctypes.c_int
    return h


def capture_fail_hook():
    """tests (BENCH_TEST_GRAPH_FAIL): a failure INSIDE a capture, as the
    8-GPU node could meet one (profiles/round5/r5f_group_tests.log:77-86): a
    hipMalloc while the stream captures (refused; it may invalidate the
    capture and leaves a sticky error), then the exception it raises."""
    import ctypes
    hip = hip_runtime()
    p = ctypes.c_void_p()
    rc = hip.hipMalloc(ctypes.byref(p), 1 << 20)
    raise CaptureHookError("graph capture refused (BENCH_TEST_GRAPH_FAIL test hook: hipMalloc under "
                           f"capture returned {rc})")


class CaptureHookError(RuntimeError):
    """capture_fail_hook's exception (the test hook's label survives the
    capture_end error that replaces it when the capture was invalidated)."""


_CAPTURE_STREAMS = []   # every capture's own HIP stream (never reused, never destroyed)


def fresh_capture_stream(torch, dev):
    """A brand-new HIP stream for one capture. A capture that fails inside
    (a hipMalloc under capture, say) leaves its stream stuck in the
    invalidated-capture state for good (HIP 7: the failed hipStreamEndCapture
    does not reset it; profiles/round6/capture_fail_probe.log), and the next
    capture begun on it cannot register torch's generator state, whose graph
    then aborts the process when destroyed. torch's default capture stream
    and its stream pool (32 streams, handed out round-robin) are both reused,
    so each capture takes a stream of its own, never handed out again."""
    import ctypes
    hip = hip_runtime()
    s = ctypes.c_void_p()
    rc = hip.hipStreamCreateWithFlags(ctypes.byref(s), ctypes.c_uint(1))   # hipStreamNonBlocking
    if rc != 0:
        raise RuntimeError(f"hipStreamCreateWithFlags: {rc}")
    _CAPTURE_STREAMS.append(s.value)
    return torch.cuda.ExternalStream(s.value, device=dev)


def recover_after_capture(torch, dev):
    """After an exception inside a capture (on its own stream: fresh_capture_
    stream): torch's __exit__ skips restoring the current stream when
    capture_end raises, so the default stream is made current again and the
    runtime's sticky error is cleared; the capture's stream is abandoned. The
    eager fallback then starts from a clean state (VERDICT r5 item 2;
    profiles/round6/capture_fail_probe.log)."""
    hip = hip_runtime()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    hip.hipGetLastError()
    try:
        torch.cuda.synchronize()
    except Exception:  # noqa: BLE001 - an error left by the failed capture
        hip.hipGetLastError()
        torch.cuda.synchronize()


def capture(torch, dev, fn, hook=False, hook_first=False):
    """A HIP graph of fn() on a capture stream of its own (returns (graph,
    fn's result)); on any failure inside the capture the state is recovered
    (recover_after_capture) before the exception propagates."""
    g = torch.cuda.CUDAGraph()
    ctx = torch.cuda.graph(g, stream=fresh_capture_stream(torch, dev))
    hooked = []
    try:
        with ctx:
            # hook_first: before fn's work (a gloo rehearsal: gloo's host
            # copies of device tensors cannot run under capture)
            out = None if (hook and hook_first) else fn()
            if hook:
                try:
                    capture_fail_hook()
                except CaptureHookError as e:
                    hooked.append(str(e))
                    raise
    except Exception as e:
        recover_after_capture(torch, dev)
        if hooked and not isinstance(e, CaptureHookError):
            # the invalidated capture's own error replaced the hook's
            raise RuntimeError(f"{hooked[0]}; then capture_end: {type(e).__name__}: "
                               f"{str(e).splitlines()[0]}") from e
        raise
    return g, out


def c_group_bucket(A, D, torch, dist, cfg, n_streams, rank, world, group, dev, wps, bits, fstride, K,
                   src, Rc, S, steps, warm, d_true, gunits, gunit, time_reps) -> dict:
    """configs[4]'s bucket through demod_group_* (one communicator per rank:
    demod_group_create with rank 0's demod_group_unique_id), timed as a HIP
    graph (eager bucket if the capture fails), every rank's frames decoded
    against the transmitted symbols, the ranks' status agreed through
    demod_group_wait. A group that cannot be created on some rank (RCCL
    refuses two ranks on one GPU) is a labelled error on every rank."""
    api = "demod_group_bucket_async (C ABI, its own RCCL communicator)"
    cg, err = None, None
    try:
        uid = None
        if world > 1:
            box = [A.group_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(box, src=0, group=group)
            uid = box[0]
        cg = A.Group(cfg, n_streams, rank=rank, world=world, uid=uid)
    except Exception as e:  # noqa: BLE001 - reported in the line
        err = f"{type(e).__name__}: {e}"[:300]
    if world > 1:
        # creation is agreed: one rank's failure is every rank's
        oks = [None] * world
        dist.all_gather_object(oks, err, group=group)
        errs = [e for e in oks if e]
        if errs and err is None:
            err = "a peer rank: " + errs[0]
    if err is not None:
        if cg is not None:
            cg.close()
        return {"error": f"demod_group_create: {err}", "api": api}
    hook = bool(os.environ.get("BENCH_TEST_GRAPH_FAIL"))
    try:
        cblock = A.group_block_bytes(n_streams, world, S, wps, bits)
        c_all = torch.zeros(cblock * world, dtype=torch.uint8, device=dev)

        def bucket():
            cg.bucket_async([src], Rc, wps, S, [c_all], [torch.cuda.current_stream().cuda_stream])
        # one eager bucket first: it sizes the group's buffers (no allocation
        # may happen under capture) and warms the communicator
        bucket()
        cg.wait([torch.cuda.current_stream().cuda_stream])
        n_rep = -(-steps // S)
        graph_error = None
        try:
            g_, _ = capture(torch, dev, bucket, hook=hook)
            c_ms = time_reps(lambda i: g_.replay(), S, n_rep, max(4, -(-warm // S)))
            how = "hip graph"
        except Exception as e:  # noqa: BLE001 - the eager bucket is timed instead
            graph_error = f"{type(e).__name__}: {e}"[:300]
            with torch.cuda.stream(torch.cuda.Stream(device=dev)):
                c_ms = time_reps(lambda i: bucket(), S, n_rep, max(2, -(-warm // S)))
                cg.wait([torch.cuda.current_stream().cuda_stream])
            how = f"eager bucket (graph capture failed: {graph_error})"
        torch.cuda.synchronize()
        cg.wait()      # every rank's status word of the last bucket (raises the agreed code)
        devs = [cg.device(0)]
        if world > 1:
            devs = [None] * world
            dist.all_gather_object(devs, cg.device(0), group=group)
        all_true = D.gather_symbols(d_true, gunits, world, unit=gunit, group=group) if world > 1 else d_true
        bad = None
        if rank == 0:
            blocks = c_all.view(world, cblock).cpu().numpy()
            tru = all_true.cpu().numpy().reshape(n_streams, wps)
            bad = 0
            for r_ in range(world):
                first, cnt = D.shard_range(n_streams, r_, world)
                for s_ in range(S):
                    for j in range(cnt):
                        off = (s_ * cnt + j) * fstride
                        back = D.unframe_symbols(A, blocks[r_][off:off + fstride].tobytes(), wps, K)
                        bad += int((back != tru[first + j]).sum())
        out = {"ms_per_step": round(c_ms, 4), "step": how, "symbol_errors": bad,
               "status": "ok (demod_group_wait: every rank's status word 0)",
               "rank_devices": devs, "distinct_devices": len(set(devs)), "world": world,
               "value": round(n_streams * wps * 1024 / (c_ms / 1e3) / 1e6, 1), "unit": "Msamples/s",
               "api": api}
        if graph_error:
            out["graph_error"] = graph_error
        return out
    except Exception as e:  # noqa: BLE001 - reported in the line
        return {"error": f"{type(e).__name__}: {e}"[:400], "api": api,
                "group_status": cg.status() if cg is not None else None}
    finally:
        cg.close()


DUMP_CAP_BYTES = 64 * 1000 * 1000   # --dump-outputs: all files together stay below this
DUMP_SEED = 0x0D0FF5


def dump_outputs(out_dir, arrays, cap=DUMP_CAP_BYTES):
    """--dump-outputs: write each (name, array) as out_dir/<name>.npy in
    float32 (float64 arrays stay float64). `array` is a numpy array or a
    device tensor, its first axis the windows. If all of them together would
    exceed `cap` bytes, every array keeps the same fraction of its rows: a
    fixed sample (sorted, drawn without replacement from a generator seeded
    with DUMP_SEED and the row count), so two builds dump the same rows.
    Returns {name: rows written}."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = [(name, a) for name, a in arrays if a is not None]

    def nbytes_as_written(a):
        per = 8 if str(a.dtype).endswith("float64") else 4
        n = 1
        for s in a.shape:
            n *= int(s)
        return n * per

    data = sum(nbytes_as_written(a) for _, a in arrays)
    head = 128 * len(arrays)   # the .npy headers
    frac = 1.0 if data + head <= cap else max(0.0, (cap - head) / float(data))
    written = {}
    for name, a in arrays:
        rows = int(a.shape[0])
        if frac < 1.0:
            keep = max(1, int(rows * frac * 0.999))
            idx = np.sort(np.random.default_rng([DUMP_SEED, rows]).choice(rows, keep, replace=False))
            a = a[idx] if isinstance(a, np.ndarray) else a[torch_like(a, idx)]
        if not isinstance(a, np.ndarray):
            a = a.cpu().numpy()
        a = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written[name] = int(a.shape[0])
    return written


def run_config(A, D, torch, dist, args, config, rank, world, local, use_dist, steps, warmup,
               plan="survey", method_name="auto", hop_fft=256, no_mags=False, spectrum=False,
               rescue_ab=False, parity_windows=0, n_streams_total=1024, sustain_s=0.0,
               parity_every=0, group=None, fft_plan="fsk2", dump_dir=None):
    """Allocate, synthesise, warm up and time one workload; returns a dict.
    fft_plan: configs[3]'s tone plan (fsk2, or fsk8: the plan-independent
    work, every post-pass block of the FFT's tones-only kernel that a
    full 8-tone plan touches). dump_dir: rank 0 writes the
    last timed step's outputs there (dump_outputs) before anything else
    touches the output buffers."""
    freqs = A.FSK8_FREQS if (config == "fsk8" or (config == "fft" and fft_plan == "fsk8")) else A.FSK2_FREQS
    if config == "fsk8" and plan == "odd":
        freqs = tuple(46.875 * (32 + 9 * i) for i in range(8))
    K = len(freqs)
    n = 1024
    method = {"auto": A.METHOD_AUTO, "goertzel": A.METHOD_GOERTZEL,
              "folded": A.METHOD_FOLDED, "residue": A.METHOD_RESIDUE}[method_name]
    hop = n
    if config == "fft":
        method, hop = A.METHOD_FFT, int(hop_fft)
    if config == "streams":
        # config 5: 1024 independent streams x 2^21 samples (2048 windows each);
        # rank r demodulates the contiguous stream shard D.shard_range(1024, r, N)
        n_streams, wps = n_streams_total, 2048
        s_first, s_count = D.shard_range(n_streams, rank, world)
        W, w0, total_windows = s_count * wps, s_first * wps, n_streams * wps
    else:
        W = int(args.windows)
        w0, total_windows = rank * W, world * W
    # windows the detector evaluates over the rank's W x n-sample stream slice
    n_eval = (W * n - n) // hop + 1
    cfg = A.make_cfg(freqs=freqs, n=n, hop=hop, device=local, method=method)
    dev = torch.device("cuda", local)
    d_pcm = torch.empty((W, n), dtype=torch.int16, device=dev)
    d_true = torch.empty(W, dtype=torch.uint8, device=dev)
    d_sym = torch.empty(n_eval, dtype=torch.uint8, device=dev)
    d_mag = None if no_mags else torch.empty((n_eval, K), dtype=torch.float32, device=dev)
    # config 4 with the full |X[b]|^2 spectrum stored (513 floats per window)
    d_spec = (torch.empty((n_eval, 513), dtype=torch.float32, device=dev)
              if (spectrum and config == "fft") else None)
    A.synth_fsk(cfg, A.BENCH_SEED, W, 8000, 400, d_pcm, d_true, w0=w0)
    torch.cuda.synchronize()
    demod = A.Demodulator(cfg)
    main = torch.cuda.current_stream()
    gunits, gunit = (n_streams, wps) if config == "streams" else (world, W)
    # With the gather: kernels run on a compute stream into double-buffered
    # symbol slots; the RCCL gather of step t-1's symbols is issued on the
    # default stream (waiting only for step t-1's kernel) and so overlaps step
    # t's kernel.
    comp = torch.cuda.Stream(device=dev) if use_dist else main
    slots = [d_sym, torch.empty_like(d_sym)] if use_dist else [d_sym]
    # config 5: every rank frames its own streams on the device (one
    # ToReceiver run per stream, demod_frame_streams_async) and RCCL gathers
    # the frames; the other configs gather symbols and rank 0 frames them.
    dev_framing = config == "streams"
    if dev_framing:
        bits = A.bits_per_symbol(K)
        fstride = A.frame_symbols_size(wps, bits)
        fslots = [torch.empty(max(s_count * fstride, 1), dtype=torch.uint8, device=dev)
                  for _ in slots]
    kdone = [torch.cuda.Event() for _ in slots]   # kernel wrote the slot
    gdone = [torch.cuda.Event() for _ in slots]   # gather finished reading the slot
    st = {"i": 0, "prev": None, "used": [False] * len(slots), "gev": None}

    def gather(slot):
        main.wait_event(kdone[slot])
        ge = st["gev"]
        if ge is not None:
            ge[0].record(main)
        if dev_framing:
            out = D.gather_symbols(fslots[slot][:s_count * fstride], gunits, world, unit=fstride,
                                   group=group)
        else:
            out = D.gather_symbols(slots[slot], gunits, world, unit=gunit, group=group)
        if ge is not None:
            ge[1].record(main)
        gdone[slot].record(main)
        return out

    def step(ev=None, gev=None):
        slot = st["i"] % len(slots)
        st["i"] += 1
        if st["used"][slot]:
            comp.wait_event(gdone[slot])
        if ev is not None:
            ev[0].record(comp)
        if d_spec is not None:
            demod.batch_spectrum_async(d_pcm, n_eval, slots[slot], d_mag, d_spec,
                                       stream=comp.cuda_stream)
        else:
            demod.batch_async(d_pcm, n_eval, slots[slot], d_mag, stream=comp.cuda_stream)
        if ev is not None:
            ev[1].record(comp)
        if dev_framing:
            A.frame_streams_async(slots[slot], s_count, wps, bits, fslots[slot],
                                  stream=comp.cuda_stream)
            if ev is not None:
                ev[2].record(comp)
        out = None
        if use_dist:
            kdone[slot].record(comp)
            st["gev"] = gev
            if st["prev"] is not None:
                out = gather(st["prev"])
            st["prev"] = slot
            st["used"][slot] = True
        return out

    def flush(gev=None):
        out = None
        if use_dist and st["prev"] is not None:
            st["gev"] = gev
            out = gather(st["prev"])
            st["prev"] = None
        return out

    def mk(k):
        return tuple(torch.cuda.Event(enable_timing=True) for _ in range(k))

    # Sustained HBM streaming shows a power-management transient: launch
    # times rise ~25 % after ~10 launches and settle back by ~60 (dispatch
    # series in profiles/round1/). Warm up for at least
    # MIN_WARMUP launches so the K timed steps see the steady state.
    warm = max(warmup, MIN_WARMUP)
    for _ in range(warm):
        step()
    flush()
    settle = None
    if not dev_framing:
        # round 6: the transient does not always end by launch 64 (a closing
        # run timed 20 steps at 0.3045 ms whose 6 s sustained rate was 0.2956,
        # profiles/round6/r6close/): further untimed warmup in chunks until
        # the per-step time has settled (settle_warmup). With the gather
        # (use_dist) every step holds a collective, so the ranks agree on
        # each chunk (all settled, or go on) and run the same number of steps
        def agree(ok):
            if world == 1:
                return ok
            t = torch.tensor([0.0 if ok else 1.0], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
            return float(t.item()) == 0.0
        n_more, settle = settle_warmup(torch, step, agree=agree, flush=flush if use_dist else None)
        warm += n_more
    timed = [i % EV_EVERY == 0 for i in range(steps)]
    evs = [mk(3) if timed[i] else None for i in range(steps)]
    gevs = [mk(2) if timed[i] else None for i in range(steps)] if use_dist else None
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        # the gather issued in step i carries step i-1's symbols
        step(evs[i], gevs[i - 1] if (gevs and i > 0) else None)
    all_sym = flush(gevs[steps - 1] if gevs else None)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    evs = [e for e in evs if e is not None]
    kts = np.array([a.elapsed_time(b) for a, b, _ in evs])
    kernel_ms = float(kts.mean())
    ms_per_step = elapsed / steps * 1e3
    frame_ms = (float(np.mean([b.elapsed_time(c) for _, b, c in evs])) if dev_framing else None)
    gdone_evs = [e for e in (gevs or []) if e is not None]
    gather_ms = (float(np.mean([a.elapsed_time(b) for a, b in gdone_evs])) if gdone_evs else None)
    ms_per_step_eager = None
    breakdown = None
    bucket = None
    c_group = None
    ring_slots = 1
    graph_hook = bool(os.environ.get("BENCH_TEST_GRAPH_FAIL"))  # tests: the capture-failure path under gloo
    ring, R = None, 1

    def time_reps(fn, S_, n_rep, n_warm):
        """ms per step of n_rep calls of fn(i) (S_ steps each) after n_warm,
        between barriers, the max over ranks"""
        for i in range(n_warm):
            fn(i)
        if world > 1:
            dist.barrier(group=group)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_rep):
            fn(i)
        if world > 1:
            dist.barrier(group=group)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
            el = float(t.item())
        return el / (n_rep * S_) * 1e3

    def time_graphs(graphs, S_, n_rep):
        return time_reps(lambda i: graphs[i % len(graphs)][0].replay(), S_, n_rep, max(4, -(-warm // S_)))

    def note(msg):
        if getattr(args, "breakdown", False):
            print(f"bench.py: streams graph: {msg}", file=sys.stderr, flush=True)

    if use_dist and dev_framing and getattr(args, "graph", False) and (args.dist_backend == "nccl" or graph_hook):
        # HIP graph of S = --graph-steps steps. The graph's
        # branches do not run concurrently (measured: a framing kernel on a
        # forked branch beside the detector adds its whole duration to the
        # step, profiles/round4/r4d/), so the step is built for that: S
        # detector launches back to back, each into its own slot of an
        # [S][windows] symbol buffer, then ONE framing launch over all S slots
        # (S x s_count "streams" of wps windows each: one ToReceiver run per
        # stream per step) and ONE RCCL all-gather of the S steps' frames: a
        # bucket of S steps per collective, so the framing launch, the
        # collective's latency (tens of us over xGMI at 8 ranks) and the graph
        # launch are paid once per S steps. S = 1 keeps round 3's step (two
        # alternating one-step graphs, framing + gather of the previous step's
        # slot on a forked branch) for the breakdown.
        S = max(1, int(getattr(args, "graph_steps", 1)))
        SB = max(S, 16 if getattr(args, "breakdown", False) else 1)   # slots for the largest bucket timed
        symS = torch.empty((SB, n_eval), dtype=torch.uint8, device=dev)
        frS = torch.empty(max(SB * s_count * fstride, 1), dtype=torch.uint8, device=dev)
        max_count = -(-n_streams // world)
        # The bucket's input ring (round 4, --ring, default): R consecutive
        # steps' batches in R slots of one buffer ([R][windows][n]), so the
        # bucket's detector work is S / R launches over R x windows each
        # instead of S launches (each launch pays its ramp and drain: 2.5 us
        # of a 77 us shard step, profiles/round4/r4g/). R is the largest
        # power of two <= S whose ring stays within --ring-gib (8 GiB): one
        # launch over 64 GiB (1024 streams, R = 16) measured slower per step
        # than 16 launches over 4 GiB (0.642 vs 0.595 ms, profiles/round4/
        # r4l/), one over 8 GiB (the 128-stream shard) faster (74.5 vs 77.5
        # us). Every slot is a copy of the synthesised batch (the symbols of
        # every step are checked below); nothing is cached between steps:
        # the ring is >= 32x the MALL.
        d_magR = None
        if getattr(args, "ring", True) and S > 1:
            cap = float(getattr(args, "ring_gib", 8.0)) * 2 ** 30
            while 2 * R <= S and S % (2 * R) == 0 and 2 * R * W * n * 2 <= cap:
                R *= 2
        ring_slots = R
        if R > 1:
            ring = torch.empty((R, W, n), dtype=torch.int16, device=dev)
            for s in range(R):
                ring[s].copy_(d_pcm)
            d_magR = None if d_mag is None else torch.empty((R * n_eval, K), dtype=torch.float32,
                                                             device=dev)
            torch.cuda.synchronize()

        def bucket_ops(kind, S_, use_ring):
            """One bucket's work on the current stream (captured into a graph,
            or run eagerly when capture fails): the detector launches, the
            framing launch, the all-gather; returns the gathered frames."""
            cs = torch.cuda.current_stream()
            if use_ring:
                for c in range(S_ // R):
                    demod.batch_async(ring, R * n_eval, symS[c * R:(c + 1) * R].reshape(-1), d_magR,
                                      stream=cs.cuda_stream)
            else:
                for s in range(S_):
                    demod.batch_async(d_pcm, n_eval, symS[s], d_mag, stream=cs.cuda_stream)
            if kind != "det":
                A.frame_streams_async(symS[:S_].reshape(-1), S_ * s_count, wps, bits, frS,
                                      stream=cs.cuda_stream)
            if kind == "full":
                return D.gather_blocks(frS[:S_ * s_count * fstride], world,
                                       S_ * max_count * fstride, group=group)
            return None

        def build_bucket(kind, S_, use_ring=False):
            # tests: BENCH_TEST_GRAPH_FAIL fails the capture from inside it
            # (test_self_launch_graph_failure_times_eager_bucket)
            return [capture(torch, dev, lambda: bucket_ops(kind, S_, use_ring),
                            hook=bool(os.environ.get("BENCH_TEST_GRAPH_FAIL")),
                            hook_first=args.dist_backend == "gloo")]

        def build_fork(kind):
            """round 3's step: two one-step graphs, framing + gather of the
            previous step's slot on a forked branch beside the detector"""
            out = []
            for sl in (0, 1):
                g = torch.cuda.CUDAGraph()
                gout = None
                with torch.cuda.graph(g):
                    cap = torch.cuda.current_stream()
                    comp.wait_stream(cap)
                    with torch.cuda.stream(comp):
                        demod.batch_async(d_pcm, n_eval, slots[sl], d_mag, stream=comp.cuda_stream)
                    if kind != "det":
                        A.frame_streams_async(slots[1 - sl], s_count, wps, bits, fslots[1 - sl],
                                              stream=cap.cuda_stream)
                    if kind == "full":
                        gout = D.gather_symbols(fslots[1 - sl][:s_count * fstride], gunits, world,
                                                unit=fstride, group=group)
                    cap.wait_stream(comp)
                out.append((g, gout))
            return out

        def time_eager_bucket(S_, n_rep):
            """The same bucket without a graph, in this process (the fallback
            when capture or replay fails)"""
            box = [None]

            def one(_i):
                box[0] = bucket_ops("full", S_, ring is not None)
            ms_ = time_reps(one, S_, n_rep, max(2, -(-warm // S_)))
            return ms_, box[0]

        ms_per_step_eager = ms_per_step
        note(f"eager {ms_per_step:.4f} ms per step; capturing the {S}-step graph")
        if S > 1:
            n_rep = -(-steps // S)
            try:
                graphs = build_bucket("full", S, use_ring=ring is not None)
                note("captured")
                # the detector's share on the same basis: a graph of the
                # bucket's detector launches alone (the full step minus it
                # is the framing + gather cost; round 4 subtracted eager
                # event times from graph replays, VERDICT r4 weak 3 iv),
                # timed interleaved with the full bucket (3 rounds each,
                # medians: one pair of back-to-back timings read -0.1 us)
                det_graphs = build_bucket("det", S, use_ring=ring is not None)
                fulls, dets = [], []
                for _ in range(3):
                    fulls.append(time_graphs(graphs, S, n_rep))
                    dets.append(time_graphs(det_graphs, S, n_rep))
                ms_per_step = float(np.median(fulls))
                note(f"timed {ms_per_step:.4f} ms per step")
                bucket = {"S": S, "gathered": graphs[0][1], "graph": True}
                bucket["det_graph_ms"] = float(np.median(dets))
            except Exception as e:  # noqa: BLE001 - the eager bucket is timed instead
                err = f"{type(e).__name__}: {e}"[:300]
                note(f"graph failed ({err}); timing the same bucket eagerly")
                # the capture's state was recovered (capture()); the eager
                # bucket runs on a fresh stream
                with torch.cuda.stream(torch.cuda.Stream(device=dev)):
                    ms_per_step, gathered = time_eager_bucket(S, n_rep)
                bucket = {"S": S, "gathered": gathered, "graph": False, "graph_error": err}
            st["i"] = None
        else:
            graphs = build_fork("full")
            n_rep = steps + 1              # + 1: the last replay gathers the last step's frames
            ms_per_step = time_graphs(graphs, 1, n_rep)
            all_sym = graphs[(n_rep - 1) % 2][1]
            st["i"] = n_rep
        if getattr(args, "breakdown", False):
            # where the step's time above the kernel goes
            def eager_det():
                demod.batch_async(d_pcm, n_eval, slots[0], d_mag, stream=comp.cuda_stream)
            breakdown = {"graph_steps": S, "ring_slots": R,
                         "eager_detector_only_ms": round(time_steps(torch, eager_det, steps, warm), 4)}
            for kind in ("det", "det_frame", "full"):
                breakdown[f"fork_1step_{kind}_ms"] = round(time_graphs(build_fork(kind), 1, steps), 4)
                note(f"fork {kind} {breakdown[f'fork_1step_{kind}_ms']}")
                for s2 in sorted({S, 8, 16} - {1}):
                    breakdown[f"bucket_{s2}step_{kind}_ms"] = round(
                        time_graphs(build_bucket(kind, s2), s2, -(-steps // s2)), 4)
                    note(f"bucket {s2} {kind} {breakdown[f'bucket_{s2}step_{kind}_ms']}")
                if ring is not None:
                    # the same bucket with its detector work as one launch over the ring
                    breakdown[f"bucket_{S}step_{kind}_ring_ms"] = round(
                        time_graphs(build_bucket(kind, S, use_ring=True), S, -(-steps // S)), 4)
                    note(f"bucket {S} {kind} ring {breakdown[f'bucket_{S}step_{kind}_ring_ms']}")
            torch.cuda.synchronize()

    if use_dist and dev_framing and getattr(args, "c_group", False):
        # the same bucket through the C ABI's RCCL group (demod_group_bucket_
        # async: detector launches, device framing, the ranks' status words
        # and frames all-gathered on its own communicator), captured and
        # replayed like the torch path's, with the same eager fallback; at
        # N > 1 this is the product's own multi-GPU path
        c_group = c_group_bucket(A, D, torch, dist, cfg, n_streams, rank, world, group, dev, wps, bits,
                                 fstride, K, ring if ring is not None else d_pcm,
                                 R if ring is not None else 1, max(1, int(getattr(args, "graph_steps", 1))),
                                 steps, warm, d_true, gunits, gunit, time_reps)

    # correctness of the timed output: every symbol vs the transmitted one
    # (sliding windows straddle two symbols: compare the aligned ones only)
    d_sym = symS[bucket["S"] - 1] if bucket else slots[(st["i"] - 1) % len(slots)]
    if hop == n:
        sym_err = int((d_sym != d_true).sum().item())
    else:
        step_w = n // hop
        sym_err = int((d_sym[::step_w][:W] != d_true).sum().item())
    dumped = None
    if dump_dir and rank == 0:
        # what a caller of the timed path holds after its last step: the
        # symbols, the tone powers and (configs[3] --spectrum) the spectrum
        dumped = dump_outputs(dump_dir, [("symbols", d_sym),
                                         ("magnitudes", d_magR[-n_eval:] if (bucket and ring is not None
                                                                             and d_magR is not None) else d_mag),
                                         ("spectrum", d_spec)])
    framed = None
    if dev_framing and bucket:
        # the last bucket's frames of every rank, every step: each must decode
        # to the transmitted symbols of its streams
        all_true = D.gather_symbols(d_true, gunits, world, unit=gunit) if world > 1 else d_true
        if rank == 0:
            blocks = bucket["gathered"].cpu().numpy()          # [world][padded block]
            tru = all_true.cpu().numpy().reshape(n_streams, wps)
            bad = 0
            for r_ in range(world):
                first, cnt = D.shard_range(n_streams, r_, world)
                for s in range(bucket["S"]):
                    for j in range(cnt):
                        off = (s * cnt + j) * fstride
                        back = D.unframe_symbols(A, blocks[r_][off:off + fstride].tobytes(), wps, K)
                        bad += int((back != tru[first + j]).sum())
            sym_err = bad
            framed = {"frames_bytes": int(sum(D.shard_range(n_streams, r_, world)[1]
                                              for r_ in range(world)) * bucket["S"] * fstride),
                      "frame_bytes_per_stream": fstride, "bits_per_symbol": bits,
                      "framing": "device (demod_frame_streams_async, %d steps per launch)" % bucket["S"],
                      "gathered": "frames of %d steps (RCCL all_gather_into_tensor, %d rank%s)"
                                  % (bucket["S"], world, "" if world == 1 else "s"),
                      "roundtrip_ok": bad == 0}
    elif dev_framing:
        # frames of the last step: gathered (with the gather) or this rank's own
        frames = all_sym if use_dist else fslots[(st["i"] - 1) % len(slots)][:s_count * fstride]
        all_true = D.gather_symbols(d_true, gunits, world, unit=gunit) if world > 1 else d_true
        if rank == 0:
            fb = frames.cpu().numpy()
            back = np.concatenate([D.unframe_symbols(A, fb[i * fstride:(i + 1) * fstride].tobytes(),
                                                     wps, K) for i in range(gunits)])
            sym_err = int((back != all_true.cpu().numpy()).sum())
            framed = {"frames_bytes": int(fb.size), "frame_bytes_per_stream": fstride,
                      "bits_per_symbol": bits, "framing": "device (demod_frame_streams_async)",
                      "gathered": ("frames (RCCL all_gather_into_tensor, %d rank%s)"
                                   % (world, "" if world == 1 else "s")) if use_dist else "no",
                      "roundtrip_ok": sym_err == 0}
    elif use_dist:
        all_true = D.gather_symbols(d_true, gunits, world, unit=gunit) if world > 1 else d_true
        sym_err = int((all_sym != all_true).sum().item())
        if rank == 0:
            # rank 0 frames the gathered symbols as ip.proto ToReceiver messages
            stream_bytes = D.frame_symbols(A, all_sym.cpu().numpy(), K)
            back = D.unframe_symbols(A, stream_bytes, all_sym.numel(), K)
            framed = {"frames_bytes": len(stream_bytes), "bits_per_symbol": A.bits_per_symbol(K),
                      "roundtrip_ok": bool((back == all_sym.cpu().numpy()).all())}

    # dispatches per step (demod_batch_launches): the detector launch (or
    # launch slices under FSKD_WB_BURSTS=0) + the rescue's; kernel_ms
    # brackets the whole batch
    launches = demod.batch_launches(n_eval, not no_mags)
    alg_bytes = W * 2 * n + n_eval * (1 + (0 if no_mags else 4 * K) +
                                      (513 * 4 if d_spec is not None else 0))
    achieved = alg_bytes / (kernel_ms / 1e3) / 1e9
    # the median launch as well as the mean (one slow
    # launch in a few moves the mean by percents)
    kernel_p50 = float(np.median(kts))
    achieved_p50 = alg_bytes / (kernel_p50 / 1e3) / 1e9
    kname = ("fft1024_quad_kernel<4>" if demod.method == A.METHOD_FFT else
             ("fold_tile_kernel<%d,4>" if demod.method == A.METHOD_FOLDED
              else "residue_tile_kernel<%d,4>" if demod.method == A.METHOD_RESIDUE
              else "goertzel_tile_kernel<%d,4>") % K)
    pmc_name = ("fsk8odd" if (config == "fsk8" and plan == "odd") else
                ("fft1024" if hop == 1024 else "fft") + ("spec" if d_spec is not None else "")
                if config == "fft" else config)
    r = {
        "config": config, "freqs": freqs, "K": K, "n": n, "hop": hop, "W": W, "n_eval": n_eval,
        "total_windows": total_windows, "ms_per_step": ms_per_step, "kernel_ms": kernel_ms,
        "kts": kts, "sym_err": sym_err, "framed": framed, "warm": warm, "settle": settle,
        "detector": {A.METHOD_GOERTZEL: "goertzel", A.METHOD_FOLDED: "folded",
                     A.METHOD_RESIDUE: "residue",
                     A.METHOD_FFT: "fft1024"}.get(demod.method, str(demod.method)),
        "roofline": {
            "bound": "hbm",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBPS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBPS, 4),
            "achieved_p50": round(achieved_p50, 1),
            "frac_p50": round(achieved_p50 / HBM_PEAK_GBPS, 4),
            "traffic": pmc_traffic(pmc_name, W, hop),
            "alg_bytes_per_launch": alg_bytes,
            "kernel": kname,
            "launches_per_step": launches,
            "timed": "the whole batch: detector launch(es) + the rescue launch (HIP events)",
        },
        "d_pcm": d_pcm, "d_sym": d_sym, "d_mag": d_mag, "d_true": d_true, "cfg": cfg,
        "spectrum": d_spec is not None, "dumped": dumped,
    }
    if dev_framing and bucket is not None and bucket.get("det_graph_ms"):
        # configs[4] on the step's own timing basis: the
        # bucket's detector launches alone, graph-replayed (per step), and the
        # whole graph step; the eager HIP-event figure stays beside them
        rf = r["roofline"]
        ach_g = alg_bytes / (bucket["det_graph_ms"] / 1e3) / 1e9
        ach_s = alg_bytes / (ms_per_step / 1e3) / 1e9
        rf.update({"achieved_eager_events": rf["achieved"], "frac_eager_events": rf["frac"],
                   "achieved": round(ach_g, 1), "frac": round(ach_g / HBM_PEAK_GBPS, 4),
                   "achieved_step": round(ach_s, 1), "frac_step": round(ach_s / HBM_PEAK_GBPS, 4),
                   "basis": "detector_graph_ms_per_step: graph replays of the bucket's detector launches "
                            "alone, per step (achieved_step: the whole graph step, ms_per_step)",
                   "timed": "graph replays (the eager HIP-event figure: achieved_eager_events)"})
    if dev_framing or use_dist:
        # per-step cost above the detector kernel: the frame
        # kernel and the gather (overlapped with the next kernel), HIP events
        r["overhead"] = {"frame_kernel_ms": round(frame_ms, 4) if frame_ms is not None else None,
                         "gather_ms": round(gather_ms, 4) if gather_ms is not None else None,
                         "step_minus_kernel_ms": round(ms_per_step - kernel_ms, 4),
                         "kernel_basis": "eager steps, HIP events around the detector batch"}
        if bucket is not None and bucket.get("det_graph_ms") is not None:
            # one timing basis: graph replays of the whole bucket vs graph
            # replays of its detector launches alone
            r["overhead"]["step_minus_kernel_ms"] = round(ms_per_step - bucket["det_graph_ms"], 4)
            r["overhead"]["detector_graph_ms_per_step"] = round(bucket["det_graph_ms"], 4)
            r["overhead"]["kernel_basis"] = ("graph replays of the bucket's detector launches alone "
                                             "(the same basis as ms_per_step)")
        if ms_per_step_eager is not None:
            r["overhead"]["ms_per_step_eager"] = round(ms_per_step_eager, 4)
            S_ = max(1, int(getattr(args, "graph_steps", 1)))
            kind = ("hip graph" if (bucket is None or bucket.get("graph")) else
                    "eager bucket (graph capture failed: %s)" % bucket.get("graph_error"))
            r["overhead"]["step"] = (
                ("%s of %d steps: %d detector launch(es), each over %d steps' batches (an input "
                 "ring of %d slots, <= %g GiB), one framing launch over the %d steps' symbol slots, one "
                 "RCCL all-gather of the %d steps' frames"
                 % (kind, S_, S_ // ring_slots, ring_slots, ring_slots, getattr(args, "ring_gib", 8.0), S_, S_))
                if S_ > 1 and ring_slots > 1
                else "%s of %d steps: %d detector launches, one framing launch over their %d "
                     "slots, one RCCL all-gather of the %d steps' frames" % (kind, S_, S_, S_, S_) if S_ > 1 else
                "hip graph per step: detector kernel on one branch; framing + RCCL gather of the "
                "previous step's symbols on the other")
            if S_ > 1:
                # launches per step in the bucket: S / R detector launches, one
                # framing launch and one collective per S steps
                r["overhead"]["launches_per_bucket"] = {"detector": S_ // ring_slots, "framing": 1,
                                                        "all_gather": 1}
                r["overhead"]["launches_per_step"] = round((S_ // ring_slots + 1) / S_, 4)
            if bucket is not None and not bucket.get("graph"):
                r["overhead"]["graph_error"] = bucket.get("graph_error")
        if breakdown is not None:
            r["overhead"]["breakdown"] = breakdown
        if c_group is not None:
            if c_group.get("ms_per_step"):
                c_group["ratio_to_torch_path"] = round(c_group["ms_per_step"] / ms_per_step, 4)
            r["overhead"]["c_group"] = c_group
    if config == "fft":
        # the FFT is reported against the VALU roof too.
        # Algorithmic flops per window: 2.5 N log2 N for the real N-point
        # FFT + 3 per |X[b]|^2 over the N/2+1 bins. Tones only, the kernel
        # runs the real split's post-pass only in the pair blocks holding a
        # tone bin (plan fft_pmask, m of 8 blocks: 64 m bins): then the
        # 512-point complex FFT's 5 (N/2) log2 (N/2) plus m/8 of the post-pass
        # (2.5 N log2 N - 5 (N/2) log2 (N/2) = 2560) and 3 per bin evaluated.
        pm = (A.plan_info(cfg)["fft_pmask"]
              if d_spec is None and os.environ.get("FSKD_FFT_PMASK") != "0" else 0xFF)
        m_blk = bin(pm & 0xFF).count("1")
        if m_blk == 8:
            fpw = 2.5 * n * 10 + 3 * (n // 2 + 1)
        else:
            fpw = 5 * (n // 2) * 9 + (2.5 * n * 10 - 5 * (n // 2) * 9 + 3 * (n // 2)) * m_blk / 8
        tf = fpw * n_eval / (kernel_ms / 1e3) / 1e12
        tf50 = fpw * n_eval / (kernel_p50 / 1e3) / 1e12
        r["roofline_valu"] = {"bound": "valu", "achieved": round(tf, 2),
                              "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                              "frac": round(tf / VALU_PEAK_TFLOPS, 4),
                              "achieved_p50": round(tf50, 2),
                              "frac_p50": round(tf50 / VALU_PEAK_TFLOPS, 4),
                              "flop_per_window": fpw,
                              "post_pass_blocks": m_blk}
    if sustain_s > 0 and not use_dist:
        # the same step back to back for sustain_s seconds (synchronised every
        # 256 steps): the steady rate over seconds rather than milliseconds,
        # long enough for an outside utilisation sampler to see the GPU busy
        torch.cuda.synchronize()
        t0, n_sus = time.perf_counter(), 0
        while True:
            for _ in range(256):
                step()
            n_sus += 256
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= sustain_s:
                break
        el = time.perf_counter() - t0
        r["sustained"] = {"seconds": round(el, 3), "steps": n_sus,
                          "ms_per_step": round(el / n_sus * 1e3, 4),
                          "value": round(total_windows * n / (el / n_sus) / 1e6, 1),
                          "unit": "Msamples/s",
                          "how": "the timed step back to back, synchronised every 256 steps"}
    # parity of the timed output itself, before the rescue A/B below reuses
    # the magnitude buffer
    if parity_every and rank == 0:
        r["parity_all"] = parity_all(d_pcm, slots[(st["i"] - 1) % len(slots)], d_mag, freqs, n, hop,
                                     config == "fft", every=parity_every)
    if parity_windows and rank == 0:
        r["parity_sample"] = parity_consecutive(A, d_pcm, slots[(st["i"] - 1) % len(slots)], d_mag,
                                                freqs, n, hop, parity_windows, config == "fft")
    if rescue_ab and not use_dist:
        # the same step with the decision rescue switched off: its cost
        os.environ["FSKD_NO_RESCUE"] = "1"
        try:
            d0 = A.Demodulator(cfg)
        finally:
            del os.environ["FSKD_NO_RESCUE"]
        sl = torch.empty_like(d_sym)

        def step0():
            if d_spec is not None:
                d0.batch_spectrum_async(d_pcm, n_eval, sl, d_mag, d_spec, stream=comp.cuda_stream)
            else:
                d0.batch_async(d_pcm, n_eval, sl, d_mag, stream=comp.cuda_stream)
        t_on, t_off = [], []
        for _ in range(3):   # interleaved: this box's drift hits both alike
            t_off.append(time_steps(torch, step0, steps, warm))
            t_on.append(time_steps(torch, lambda: step(), steps, warm))
        on, off = float(np.median(t_on)), float(np.median(t_off))
        # how many windows the detector flagged: a handle that flags but
        # skips the rescue launch leaves bit 7 on those symbols
        os.environ["FSKD_NO_RESCUE"] = "flags"
        try:
            df = A.Demodulator(cfg)
        finally:
            del os.environ["FSKD_NO_RESCUE"]
        if d_spec is not None:
            df.batch_spectrum_async(d_pcm, n_eval, sl, d_mag, d_spec, stream=comp.cuda_stream)
        else:
            df.batch_async(d_pcm, n_eval, sl, d_mag, stream=comp.cuda_stream)
        torch.cuda.synchronize()
        flagged = int((sl >= 128).sum().item())
        df.close()
        r["rescue"] = {"ms_per_step": round(on, 4), "ms_per_step_without_rescue": round(off, 4),
                       "cost_frac": round((on - off) / off, 4),
                       "flagged_windows": flagged, "flagged_frac": flagged / float(n_eval),
                       "launches_without": d0.batch_launches(n_eval, not no_mags),
                       "how": "interleaved medians of 3 x %d steps each way" % steps}
        d0.close()
        del sl
    demod.close()
    return r


def settle_warmup(torch, fn, chunk=16, max_chunks=32, tol=0.01, agree=None, flush=None):
    """Untimed warmup past the clock transient: chunks of `chunk` steps, each
    timed (synchronised), until two consecutive chunks agree within tol and
    the last is within 3 % of the fastest chunk seen (at most max_chunks,
    ~0.15 s at configs[1]). agree(settled) -> bool makes the stop decision
    common to every rank (the steps hold collectives); flush() ends a chunk's
    pending gather. Returns (steps run, per-chunk ms per step)."""
    times = []
    for _ in range(max_chunks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(chunk):
            fn()
        if flush is not None:
            flush()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / chunk * 1e3)
        ok = (len(times) >= 2 and abs(times[-1] - times[-2]) <= tol * times[-1]
              and times[-1] <= 1.03 * min(times))
        if agree is not None:
            ok = agree(ok)
        if ok:
            break
    return len(times) * chunk, [round(t, 4) for t in times]


def time_steps(torch, fn, steps, warm) -> float:
    """ms per step of `fn` over `steps` launches after `warm` (synchronised)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def parity_consecutive(A, d_pcm, d_sym, d_mag, freqs, n, hop, count, fft):
    """GPU vs the oracle on the first `count` consecutive windows of the timed
    output (at hop < n these include every window straddling two symbols):
    symbol mismatches, windows whose oracle top-2 margin is inside the fp32
    band (decided by the rescue), magnitude error relative to max_k P and the
    count of windows above 1e-5 of max_k P."""
    sys.path.insert(0, ROOT)
    from oracle import oracle as O
    W = min(count, d_sym.numel())
    flat = d_pcm.reshape(-1)[:(W - 1) * hop + n].cpu().numpy()
    _, _, _, threads, _ = cpu_share()
    if fft:
        sym, P = O.fft_demod(flat, freqs, n, hop, threads=threads)
    else:
        sym, P = O.goertzel(flat, freqs, n, hop, threads=threads)
    gs = d_sym[:W].cpu().numpy()
    out = {"windows_checked": int(W), "consecutive": True, "hop": hop,
           "oracle": "oracle_fft_demod (double radix-2)" if fft else "oracle_goertzel (double)",
           "symbol_mismatches": int((gs != sym).sum()),
           "flag_bits_left": int(((gs & 0x80) != 0).sum()),
           "margin": margin_stats(P)}
    if d_mag is not None:
        gm = d_mag[:W].cpu().numpy().astype(np.float64)
        rel = np.abs(gm - P).max(1) / np.maximum(P.max(1), 1e-300)
        out["max_rel_mag_err"] = float(rel.max())
        out["windows_above_1e-5_of_max_P"] = int((rel > 1e-5).sum())
        x = flat.astype(np.float64)
        c2 = np.concatenate([[0.0], np.cumsum(x * x)])
        st_ = np.arange(W) * hop
        energy = n * (c2[st_ + n] - c2[st_]) / 2
        out["max_mag_err_of_energy"] = float((np.abs(gm - P).max(1) / np.maximum(energy, 1e-300)).max())
    return out


def parity_all(d_pcm, d_sym, d_mag, freqs, n, hop, fft, every=1, chunk=65536):
    """GPU vs the oracle on every `every`-th window of the whole timed output
    (every = 1: all of them), in chunks of `chunk` windows: symbol
    mismatches, flag bits left, magnitude error relative to max_k P and the
    count of windows above 1e-5 of max_k P."""
    sys.path.insert(0, ROOT)
    from oracle import oracle as O
    _, _, _, threads, _ = cpu_share()
    W = d_sym.numel()
    flat = d_pcm.reshape(-1)
    idx_all = np.arange(0, W, every)
    mism = flags = above = 0
    worst = 0.0
    t0 = time.perf_counter()
    for c0 in range(0, idx_all.size, chunk):
        idx = idx_all[c0:c0 + chunk]
        if every == 1:
            a, b = int(idx[0]), int(idx[-1])
            x = flat[a * hop:b * hop + n].cpu().numpy()
            oh = hop
        else:
            # the sampled windows side by side, each its own n samples
            starts = torch_index(flat, idx, hop, n)
            x, oh = starts, n
        if fft:
            sym, P = O.fft_demod(x, freqs, n, oh, threads=threads)
        else:
            sym, P = O.goertzel(x, freqs, n, oh, threads=threads)
        ii = torch_like(d_sym, idx)
        gs = d_sym[ii].cpu().numpy()
        mism += int((gs != sym).sum())
        flags += int(((gs & 0x80) != 0).sum())
        if d_mag is not None:
            gm = d_mag[ii].cpu().numpy().astype(np.float64)
            rel = np.abs(gm - P).max(1) / np.maximum(P.max(1), 1e-300)
            worst = max(worst, float(rel.max()))
            above += int((rel > 1e-5).sum())
    out = {"windows_checked": int(idx_all.size), "of_windows": int(W),
           "sample": "every window" if every == 1 else f"every {every}th window",
           "oracle": "oracle_fft_demod (double radix-2)" if fft else "oracle_goertzel (double)",
           "symbol_mismatches": mism, "flag_bits_left": flags,
           "oracle_seconds": round(time.perf_counter() - t0, 2), "threads": threads}
    if d_mag is not None:
        out["max_rel_mag_err"] = worst
        out["windows_above_1e-5_of_max_P"] = above
    return out


def torch_like(t, idx):
    import torch
    return torch.as_tensor(idx, device=t.device)


def torch_index(flat, idx, hop, n):
    """The n samples of each window in idx, gathered on the device, as one
    contiguous host array (window after window)."""
    import torch
    off = torch.as_tensor(idx, device=flat.device)[:, None] * hop + torch.arange(n, device=flat.device)
    return flat[off.reshape(-1)].cpu().numpy()


def summary(r) -> dict:
    """The extra-config entry of the bench line."""
    out = {"workload": (f"configs[2]: 8-FSK Goertzel, {r['W']} x 1024 windows" if r["config"] == "fsk8"
                        else f"configs[3]: sliding 1024-pt FFT, hop {r['hop']}, {r['n_eval']} windows, "
                        f"{r['K']}-tone plan {list(r['freqs'])}"
                        + (", full |X[b]|^2 spectrum stored (513 floats per window)"
                           if r.get("spectrum") else "")),
           "detector": r["detector"], "ms_per_step": round(r["ms_per_step"], 4),
           "kernel_ms": round(r["kernel_ms"], 4),
           "kernel_ms_p10_p50_p90": [round(float(np.percentile(r["kts"], q)), 4) for q in (10, 50, 90)],
           "value": round(r["W"] * 1024 / (r["ms_per_step"] / 1e3) / 1e6, 1), "unit": "Msamples/s",
           "symbol_errors": r["sym_err"],
           "launches_per_step": r["roofline"]["launches_per_step"]}
    for key in ("rescue", "parity_sample", "parity_all"):
        if key in r:
            out[key] = r[key]
    if r["config"] == "fft":
        out["roofline"] = r["roofline_valu"]
        # HBM: the unique input stream plus the outputs (with the spectrum:
        # 2052 B per window written, the larger stream)
        out["roofline_hbm_frac"] = round(
            r["roofline"]["alg_bytes_per_launch"] / (r["kernel_ms"] / 1e3) / 1e9 / HBM_PEAK_GBPS, 4)
        out["roofline_hbm_frac_p50"] = r["roofline"]["frac_p50"]
        out["hbm_alg_bytes_per_launch"] = r["roofline"]["alg_bytes_per_launch"]
        out["hbm_traffic"] = r["roofline"]["traffic"]
    else:
        out["roofline"] = r["roofline"]
    return out


def streams_child(args, n_streams: int = 1024, breakdown: bool = False) -> dict:
    """configs[4] at N = 1 as the 8-GPU run's step takes it: a child
    `bench.py --config streams --force-dist` (RCCL at world size 1, one HIP
    graph per step), its line reduced to the entry of this one. n_streams =
    128 is the shard one rank of the 8-GPU run gets."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    cmd = [sys.executable, "-u", os.path.abspath(__file__), "--config", "streams", "--force-dist",
           "--streams-total", str(n_streams), "--graph-steps", str(args.graph_steps),
           # >= 16 replays of the 16-step graph: 2 replays (the driver's
           # --steps 20) left the shard's rate within +-7 % run to run (r4g)
           "--steps", str(max(args.steps, 256)), "--warmup", str(args.warmup), "--no-cpu-baseline"]
    if breakdown:
        cmd.append("--breakdown")
    elif n_streams == 1024:
        cmd.append("--c-group")   # the same bucket through the C ABI's RCCL group, beside it
    r = subprocess.run(cmd, capture_output=True, timeout=600, cwd=ROOT, env=env)
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": f"rc {r.returncode}", "stderr_tail": r.stderr.decode()[-800:]}
    ln = json.loads(lines[-1])
    keep = ("value", "unit", "ms_per_step", "kernel_ms", "kernel_ms_p10_p50_p90", "symbol_errors",
            "overhead", "framing", "roofline", "rescue", "scaling", "n_gpus")
    out = {k: ln[k] for k in keep if k in ln}
    out["workload"] = ln["config"]["workload"]
    out["how"] = ("child: bench.py --config streams --force-dist --streams-total %d (nccl, world size "
                  "1, graph step)" % n_streams)
    return out


def host_e2e(A, torch, r, reps=5) -> dict:
    """The PCIe-inclusive path (never the headline value): the headline's 2 GiB
    of windows from a pageable host array through demod_batch (chunked H2D on a
    copy stream, kernels behind each chunk, results back), against the raw
    host-to-device copy rate of the same bytes (pageable and pinned)."""
    x = r["d_pcm"].cpu().numpy()
    W, nbytes = x.shape[0], x.nbytes
    with A.Demodulator(r["cfg"]) as d:
        sym, mag = d.batch(x, mags=True)                 # warm: allocations, first copies
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            sym, mag = d.batch(x, mags=True)
            t.append(time.perf_counter() - t0)
    tb = float(np.median(t))
    src = torch.from_numpy(x)
    pin = src.pin_memory()
    dst = torch.empty_like(r["d_pcm"])
    rates = {}
    for name, h in (("pageable", src), ("pinned", pin)):
        dst.copy_(h)
        torch.cuda.synchronize()
        tt = []
        for _ in range(reps):
            t0 = time.perf_counter()
            dst.copy_(h)
            torch.cuda.synchronize()
            tt.append(time.perf_counter() - t0)
        rates[name] = nbytes / float(np.median(tt)) / 1e9
    true_sym = r["d_true"].cpu().numpy() if "d_true" in r else None
    gbps = nbytes / tb / 1e9
    out = {"workload": f"configs[1] windows from a pageable host buffer ({nbytes} B), demod_batch "
                       "host pointers: symbols + |X_k|^2 back in host memory",
           "ms_per_batch": round(tb * 1e3, 3), "GB_per_s": round(gbps, 2),
           "Msamples_per_s": round(W * 1024 / tb / 1e6, 1),
           "h2d_GB_per_s": {k: round(v, 2) for k, v in rates.items()},
           "frac_of_pageable_h2d": round(gbps / rates["pageable"], 4),
           "symbols_equal_device_path": bool((sym == r["d_sym"].cpu().numpy()).all()),
           "reps": reps}
    if true_sym is not None:
        out["symbol_errors"] = int((sym != true_sym).sum())
    del pin, dst
    return out


def two_tone_stream(torch, d_pcm, freqs, a, b, amp=12000.0, sigma=1.0, seed=7):
    """The worst case of the decision rescue: a continuous
    stream x[g] = amp (sin(w_a g) + sin(w_b g + phi)) + N(0, sigma), two tones
    of the plan at equal power (integer bins: every window, at any hop that is
    a multiple of 8, holds both tones at equal power up to the noise and the
    int16 rounding, so every window is within the rescue's threshold).
    Written into d_pcm ([W][n] int16, device) in chunks, in float64 on the
    device."""
    flat = d_pcm.reshape(-1)
    gen = torch.Generator(device=d_pcm.device)
    gen.manual_seed(seed)
    wa = 2 * math.pi * freqs[a] / 48000.0
    wb = 2 * math.pi * freqs[b] / 48000.0
    chunk = 1 << 25
    for c0 in range(0, flat.numel(), chunk):
        c1 = min(flat.numel(), c0 + chunk)
        g = torch.arange(c0, c1, device=d_pcm.device, dtype=torch.float64)
        v = amp * (torch.sin(torch.remainder(g * wa, 2 * math.pi)) +
                   torch.sin(torch.remainder(g * wb, 2 * math.pi) + 1.234))
        v += sigma * torch.randn(c1 - c0, device=d_pcm.device, dtype=torch.float64, generator=gen)
        flat[c0:c1] = torch.clamp(torch.round(v), -32768, 32767).to(torch.int16)
    torch.cuda.synchronize()


def rescue_worst(A, torch, steps, warm, W=1 << 20) -> dict:
    """Every window ambiguous: the rescue's cost bound per detector, 2^20
    windows of the two-tone worst case (two_tone_stream): 2-FSK (plain bank,
    rescue inside the kernel), 8-FSK (fold F16, inside the kernel), FFT hop
    256 over the same 2^30-sample stream (inside the kernel), 2-FSK and 8-FSK
    at hop 256 (segment-shared windows, SLIDE / fold-slide: the rescue
    launch), 8-FSK on bins 32 + 9 i (the residue detector). Per detector the
    step with the rescue (shipped), without it (FSKD_NO_RESCUE=1), with its
    exact path only (FSKD_RESCUE_SEG=0: no first pass by segments), the
    flagged fraction (FSKD_NO_RESCUE=flags) and a parity sample of the first
    4096 windows against the oracle (every symbol must be the oracle's)."""
    sys.path.insert(0, ROOT)
    from oracle import oracle as O
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 1024
    d_pcm = torch.empty((W, n), dtype=torch.int16, device=dev)
    out = {"workload": f"{W} x 1024-sample windows, two plan tones at equal power in every window "
                       "(continuous, amplitude 12000 each, sigma 1 noise)"}
    for key, freqs, a, b, method, hop in (("fsk2", A.FSK2_FREQS, 0, 1, A.METHOD_AUTO, n),
                                          ("fsk8", A.FSK8_FREQS, 2, 5, A.METHOD_AUTO, n),
                                          ("fft_hop256", A.FSK8_FREQS, 2, 5, A.METHOD_FFT, 256),
                                          # segment-shared windows: the rescue launch
                                          ("fsk2_slide_hop256", A.FSK2_FREQS, 0, 1, A.METHOD_AUTO,
                                           256),
                                          # fold-slide: the rescue launch, pass 0 by the fold
                                          ("fsk8_slide_hop256", A.FSK8_FREQS, 2, 5, A.METHOD_AUTO,
                                           256),
                                          # 8 tones on bins 32 + 9 i: the residue detector,
                                          # pass 0 by segments
                                          ("fsk8odd", tuple(46.875 * (32 + 9 * i) for i in range(8)),
                                           2, 5, A.METHOD_AUTO, n)):
        two_tone_stream(torch, d_pcm, freqs, a, b)
        n_eval = (W * n - n) // hop + 1
        K = len(freqs)
        sym = torch.empty(n_eval, dtype=torch.uint8, device=dev)
        mag = torch.empty((n_eval, K), dtype=torch.float32, device=dev)
        cfg = A.make_cfg(freqs=freqs, n=n, hop=hop, method=method)
        res = {}
        # modes: flags only (count), no rescue, the exact path only (the
        # rescue's first pass off, FSKD_RESCUE_SEG=0), shipped (last: its
        # symbols are the parity sample's)
        for mode in ("flags", "1", "exact", None):
            var = "FSKD_RESCUE_SEG" if mode == "exact" else "FSKD_NO_RESCUE"
            if mode is not None:
                os.environ[var] = "0" if mode == "exact" else mode
            try:
                d = A.Demodulator(cfg)
            finally:
                os.environ.pop(var, None)
            with d:
                if mode == "flags":
                    d.batch_device(d_pcm, n_eval, sym, mag)
                    res["flagged_frac"] = round(float((sym >= 128).sum().item()) / n_eval, 6)
                    continue
                fn = (lambda: d.batch_async(d_pcm, n_eval, sym, mag))
                t = time_steps(torch, fn, max(10, steps // 4), max(4, warm // 8))
                res[{None: "ms_per_step", "1": "ms_per_step_without_rescue",
                     "exact": "ms_per_step_exact_path_only"}[mode]] = round(t, 4)
                res["detector"] = {A.METHOD_GOERTZEL: "goertzel", A.METHOD_FOLDED: "folded",
                                   A.METHOD_RESIDUE: "residue", A.METHOD_FFT: "fft1024"}.get(d.method)
                res["launches_per_step"] = d.batch_launches(n_eval, True)
        S = 4096
        x = d_pcm.reshape(-1)[:(S - 1) * hop + n].cpu().numpy()
        rs, _ = (O.fft_demod if method == A.METHOD_FFT else O.goertzel)(x, freqs, n, hop=hop, threads=16)
        gs = sym[:S].cpu().numpy()
        res["parity_sample"] = {"windows": S, "symbol_mismatches": int((gs != rs).sum())}
        res["slowdown"] = round(res["ms_per_step"] / res["ms_per_step_without_rescue"], 3)
        res["Msamples_per_s"] = round(W * n / (res["ms_per_step"] / 1e3) / 1e6, 1)
        out[key] = res
        del sym, mag
    del d_pcm
    torch.cuda.empty_cache()
    return out


def quiet_cost(A, torch, steps, warm, W=1 << 20) -> dict:
    """The detectors on quiet input (round 3 flagged every window
    of it): digital silence (all zeros) and dithered silence (Gaussian sigma
    3, rounded), 2^20 windows each; per detector the step's time against the
    same detector on the bench's FSK stream, and the flagged fraction
    (FSKD_NO_RESCUE=flags). Digital silence is decided without a rescue; the
    P_max == 0 candidates of stage 1 only cost the energy test."""
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 1024
    d_pcm = torch.empty((W, n), dtype=torch.int16, device=dev)
    d_true = torch.empty(W, dtype=torch.uint8, device=dev)
    out = {"workload": f"{W} x 1024-sample windows: FSK (bench stream), digital silence, dithered "
                       "silence (sigma 3)"}
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    for key, freqs, method, hop in (("fsk2", A.FSK2_FREQS, A.METHOD_AUTO, n),
                                    ("fsk8", A.FSK8_FREQS, A.METHOD_AUTO, n),
                                    ("fft_hop256", A.FSK8_FREQS, A.METHOD_FFT, 256)):
        n_eval = (W * n - n) // hop + 1
        K = len(freqs)
        sym = torch.empty(n_eval, dtype=torch.uint8, device=dev)
        mag = torch.empty((n_eval, K), dtype=torch.float32, device=dev)
        cfg = A.make_cfg(freqs=freqs, n=n, hop=hop, method=method)
        res = {}
        for inp in ("fsk", "zeros", "dither3"):
            if inp == "fsk":
                A.synth_fsk(cfg, A.BENCH_SEED, W, 8000, 400, d_pcm, d_true)
            elif inp == "zeros":
                d_pcm.zero_()
            else:
                d_pcm.copy_(torch.round(3.0 * torch.randn((W, n), device=dev, generator=gen)).to(torch.int16))
            torch.cuda.synchronize()
            os.environ["FSKD_NO_RESCUE"] = "flags"
            try:
                d = A.Demodulator(cfg)
            finally:
                os.environ.pop("FSKD_NO_RESCUE", None)
            with d:
                d.batch_device(d_pcm, n_eval, sym, mag)
                flagged = float((sym >= 128).sum().item()) / n_eval
            with A.Demodulator(cfg) as d:
                # past the clock transient of the first ~60 launches (MIN_WARMUP)
                t = time_steps(torch, lambda: d.batch_async(d_pcm, n_eval, sym, mag),
                               max(40, steps), max(MIN_WARMUP, warm))
                if inp == "zeros":
                    zeros_ok = bool((sym == 0).all().item())
            res[inp] = {"ms_per_step": round(t, 4), "flagged_frac": round(flagged, 6)}
        res["zeros"]["all_tone_0"] = zeros_ok
        out[key] = res
        del sym, mag
    del d_pcm, d_true
    torch.cuda.empty_cache()
    return out


def error_model_headroom(A) -> dict:
    """The decision rescue's error model on the shipped configurations
    (tests/error_model.py; the full sweep is tests/test_gpu_error_model.py):
    per detector the worst fp32 power error over every adversarial family as a
    fraction of tau sqrt(P_max NE), the rescue's margin threshold (the model
    allows 1/12), whether the flags are exactly the stated threshold's and
    whether every unflagged window carries the oracle's symbol."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import oracle as O
    import error_model as EM
    out = {"families": EM.FAMILIES, "windows_per_family": 4096}
    worst = 0.0
    for case in EM.CASES:
        if case[0] not in ("plain_k2", "fold_f16_k8", "fft_h256_k8", "residue_dcls_k8"):
            continue
        rows = [EM.evaluate(A, O, case, fam, W=4096) for fam in EM.FAMILIES]
        w = max(rows, key=lambda r: r["worst_err_frac_of_tau"])
        out[case[0]] = {"tau": rows[0]["tau"],
                        "worst_err_frac_of_tau": round(w["worst_err_frac_of_tau"], 5),
                        "at_family": w["family"],
                        "worst_ratio_to_model": round(max(r["worst_ratio_to_model"] for r in rows), 4),
                        "flags_exact": all(r["flag_missed"] == 0 and r["flag_extra"] == 0 for r in rows),
                        "unflagged_wrong": sum(r["unflagged_wrong"] for r in rows),
                        "quiet_flagged_frac": [r["flagged"] / r["windows"] for r in rows
                                               if r["family"] == "quiet_s3"][0]}
        worst = max(worst, w["worst_err_frac_of_tau"])
    out["worst_err_frac_of_tau"] = round(worst, 5)
    out["implied_mag_bound"] = implied_mag_bounds(A)
    return out


def implied_mag_bound(A, cfg) -> dict:
    """The magnitude error the derived bounds imply, for a
    window whose strongest tone carries its energy, |X_max|^2 = n sum x^2 / 2
    (an aligned FSK symbol): with a = rho_det sqrt(E_det) + rho_ref sqrt(sum
    x^2) bounding |sqrt(P_k) - sqrt(P_ref,k)| (demod_error_model; E_det <= 8
    sum x^2 for the fold detector's folded window, Cauchy-Schwarz), every tone
    has |P_k - P_ref,k| / P_max <= 2 a' + a'^2, a' = a / |X_max|. The bar is
    north_star's 1e-5 relative."""
    m = A.error_model(cfg)
    f = 8.0 if m["energy"] == A.ENERGY_FOLDED else 1.0
    a = (m["rho_det"] * f ** 0.5 + m["rho_ref"]) * (2.0 / cfg.n) ** 0.5
    b = 2 * a + a * a
    det = {A.METHOD_GOERTZEL: "goertzel", A.METHOD_FOLDED: "folded", A.METHOD_RESIDUE: "residue",
           A.METHOD_FFT: "fft1024"}.get(m["method"], str(m["method"]))
    return {"detector": det, "rho_det": m["rho_det"], "energy": m["energy"], "bound": float("%.4g" % b),
            "within_1e-5": b <= 1e-5}


def implied_mag_bounds(A) -> dict:
    """implied_mag_bound per shipped configuration (AUTO's detector), and the
    fold detector on configs[1]'s plan (DEMOD_METHOD_FOLDED: derived < 1e-5,
    at ~2 % of the step)."""
    fsk2, fsk8 = A.FSK2_FREQS, A.FSK8_FREQS
    out = {
        "configs[1]": implied_mag_bound(A, A.make_cfg(freqs=fsk2)),
        "configs[1]_method_folded": implied_mag_bound(A, A.make_cfg(freqs=fsk2, method=A.METHOD_FOLDED)),
        "configs[2]": implied_mag_bound(A, A.make_cfg(freqs=fsk8)),
        "configs[3]_fsk2_hop256": implied_mag_bound(A, A.make_cfg(freqs=fsk2, hop=256, method=A.METHOD_FFT)),
        "configs[3]_fsk8_hop256": implied_mag_bound(A, A.make_cfg(freqs=fsk8, hop=256, method=A.METHOD_FFT)),
        "configs[4]": implied_mag_bound(A, A.make_cfg(freqs=fsk2)),
    }
    out["note"] = ("configs[1] / [4] under AUTO (the plain bank) carry a derived bound of ~7e-5: their 1e-5 "
                   "magnitude bar is MEASURED on every timed window (parity_all), not implied by the "
                   "analysis; DEMOD_METHOD_FOLDED implies it (8.8e-6)")
    return out


def comm_info(torch, dist, local, backend) -> dict:
    """The communicator's world and every rank's device (PCI address, UUID),
    gathered from all ranks (a collective: every rank calls it)."""
    p = torch.cuda.get_device_properties(local)
    me = {"rank": dist.get_rank(), "local_rank": local, "device": p.name,
          "pci": "%04x:%02x:%02x" % (getattr(p, "pci_domain_id", 0), getattr(p, "pci_bus_id", 0),
                                     getattr(p, "pci_device_id", 0)),
          "uuid": str(getattr(p, "uuid", ""))}
    ranks = [None] * dist.get_world_size()
    dist.all_gather_object(ranks, me)
    ver = None
    if backend == "nccl":
        try:
            v = torch.cuda.nccl.version()
            ver = ".".join(str(x) for x in v) if isinstance(v, tuple) else str(v)
        except Exception:  # noqa: BLE001
            ver = None
    return {"backend": "nccl (RCCL)" if backend == "nccl" else backend,
            "world_size": dist.get_world_size(), "ranks": ranks,
            "distinct_devices": len({(r["pci"], r["uuid"]) for r in ranks}),
            "rccl_version": ver}


def self_launch(args) -> int:
    """--gpus N > 1 without WORLD_SIZE: run N ranks under torch.distributed.run
    (a child process started before this one touches the GPU); rank 0's line
    is printed by the child."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", "--master-addr=127.0.0.1",
           f"--master-port={free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", choices=["fsk2", "fsk8", "fft", "streams"], default="fsk2",
                    help="fsk2 = configs[1] (default), fsk8 = configs[2], fft = configs[3]: "
                         "sliding 1024-pt full-spectrum FFT (hop --hop) over the same stream, "
                         "streams = configs[4]: 1024 streams x 2048 windows sharded over ranks "
                         "(strong scaling)")
    ap.add_argument("--hop", type=int, default=256, help="window advance for --config fft")
    ap.add_argument("--streams-total", type=int, default=1024,
                    help="--config streams: streams in the whole job (configs[4]: 1024; 128 = one "
                         "rank's shard at 8 GPUs)")
    ap.add_argument("--windows", type=int, default=1 << 20, help="windows per GPU (fsk2/fsk8)")
    ap.add_argument("--no-mags", action="store_true", help="symbols only")
    ap.add_argument("--spectrum", action="store_true",
                    help="--config fft: also store the full |X[b]|^2 spectrum (513 floats per window)")
    ap.add_argument("--method", choices=["auto", "goertzel", "folded", "residue"], default="auto")
    ap.add_argument("--plan", choices=["survey", "odd"], default="survey",
                    help="fsk8 tone plan: survey = SURVEY §8 (1500 + 375 i Hz, multiples of 8 "
                         "bins), odd = integer bins 32 + 9 i (every residue class mod 8: the "
                         "generic integer-bin path, DESIGN.md §4.3)")
    ap.add_argument("--cpu-seconds", type=float, default=14.0)
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the extra entries (fsk8, fft_hop256*, streams, host_e2e at N = 1; "
                         "streams at N > 1)")
    ap.add_argument("--no-rescue-ab", action="store_true",
                    help="skip the rescue-off A/B runs (profiling: only the shipped path launches)")
    ap.add_argument("--sustain", type=float, default=6.0,
                    help="N = 1 headline: also run the step back to back for this many seconds "
                         "and report the rate as 'sustained' (0: off)")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise torch.distributed and run the gather even at N = 1 "
                         "(exercises the RCCL path on one GPU)")
    ap.add_argument("--no-graph", dest="graph", action="store_false",
                    help="streams config: time eager steps instead of HIP graphs")
    ap.add_argument("--graph-steps", type=int, default=16,
                    help="streams config: steps per HIP graph and per framing launch + RCCL gather "
                         "(a bucket of S steps); 1: round 3's step, one graph per step with the "
                         "previous step's framing + gather on a forked branch")
    ap.add_argument("--ring-gib", type=float, default=8.0,
                    help="configs[4] graph bucket: the input ring's size cap (one detector launch per ring)")
    ap.add_argument("--no-ring", dest="ring", action="store_false",
                    help="configs[4] graph bucket: S detector launches over one input buffer instead "
                         "of one launch over an S-slot input ring")
    ap.add_argument("--c-group", action="store_true",
                    help="streams config: also time the same bucket through the C ABI's RCCL group "
                         "(demod_group_bucket_async) and report it beside the torch path (always on "
                         "for the N > 1 configs[4] extra unless --no-c-group)")
    ap.add_argument("--no-c-group", action="store_true",
                    help="N > 1: skip timing the configs[4] bucket through the C ABI's RCCL group "
                         "(demod_group_*) beside the torch path")
    ap.add_argument("--breakdown", action="store_true",
                    help="streams config: also time the step's pieces (detector alone, graphs "
                         "without the gather / framing, 1 / S / 8 steps per graph)")
    ap.add_argument("--extras-only", default="",
                    help="comma-separated subset of the default line's extras (measurement calls): "
                         "fsk8, fft_hop256, fft_hop256_fsk8, fft_hop256_spectrum, host_e2e, error_model, rescue_worst, "
                         "quiet_cost, streams")
    ap.add_argument("--extras-timeout", type=float, default=240.0,
                    help="N > 1: seconds the configs[4] extra may take before a watchdog prints "
                         "the headline line without it and ends every rank")
    ap.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl",
                    help="nccl (= RCCL over xGMI) on the real node; gloo only to rehearse the "
                         "multi-rank path with several ranks sharing one GPU")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline figure: the CPU "
                         "baseline and its parity samples, parity of every timed window, the rescue "
                         "A/B, the sustained rate and the extra entries (other configs, host_e2e, "
                         "error_model, rescue_worst, quiet_cost, streams; at N > 1 configs[4]). "
                         "Without it the run sets up, warms up, times --steps steps and prints its line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed step's outputs (rank 0: symbols, "
                         "magnitudes, and the spectrum with --spectrum) as DIR/<name>.npy in float32, at "
                         "most 64 MB in all (a fixed seeded sample of the rows beyond that)")
    args = ap.parse_args()
    if not args.full:
        if args.extras_only:
            ap.error("--extras-only picks among the entries of --full: add --full")
        # the headline figure alone: no CPU baseline or parity pass, no rescue
        # A/B, no sustained run, no extra entries
        args.no_cpu_baseline = args.no_extras = args.no_rescue_ab = True
        args.sustain = 0.0

    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(self_launch(args))
    world = int(env_world or "1")
    if world != args.gpus and not (world == 1 and args.gpus == 1):
        print(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus}", file=sys.stderr)
        sys.exit(2)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    import torch

    if args.dist_backend == "gloo":
        local = local % torch.cuda.device_count()  # rehearsal: ranks may share a GPU
    torch.cuda.set_device(local)
    use_dist = world > 1 or args.force_dist
    dist = None
    if use_dist:
        import torch.distributed as dist
        init = {}
        if world == 1 and "MASTER_PORT" not in os.environ:
            init = {"init_method": f"tcp://127.0.0.1:{free_port()}", "rank": 0, "world_size": 1}
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local), **init)
        else:
            dist.init_process_group("gloo", **init)

    A, D = load_pkg()
    plain = world == 1 and not args.force_dist and args.method == "auto" and not args.no_mags
    r = run_config(A, D, torch, dist, args, args.config, rank, world, local, use_dist,
                   args.steps, args.warmup, plan=args.plan, method_name=args.method,
                   n_streams_total=args.streams_total,
                   hop_fft=args.hop, no_mags=args.no_mags, spectrum=args.spectrum,
                   rescue_ab=plain and args.config in ("fsk2", "fsk8", "fft") and not args.no_rescue_ab,
                   sustain_s=args.sustain if plain and args.config == "fsk2" and not args.no_extras else 0.0,
                   parity_every=1
                   if plain and not args.no_cpu_baseline else 0, dump_dir=args.dump_outputs)

    extras = {}
    guard = None
    if world > 1:
        # what the collective ran on: every rank's device
        extras["rccl"] = comm_info(torch, dist, local, args.dist_backend)
    if plain and args.config == "fsk2" and not args.no_extras:
        # configs[2] and configs[3], same warmup, in their own buffers
        # (the main run's stay alive for the CPU baseline's parity sample)
        main_keep = {k: r[k] for k in ("d_pcm", "d_sym", "d_mag", "d_true")}
        only = set(args.extras_only.split(",")) if args.extras_only else None

        def want(key):  # --extras-only: a measurement call's subset of the extras
            return only is None or key in only
        for key, cfgname, spec, fplan in (("fsk8", "fsk8", False, "fsk2"), ("fft_hop256", "fft", False, "fsk2"),
                                          ("fft_hop256_fsk8", "fft", False, "fsk8"),
                                          ("fft_hop256_spectrum", "fft", True, "fsk2")):
            if not want(key):
                continue
            # >= 100 timed steps (>= 25 event-timed launches): at the driver's
            # --steps 20 the kernel mean rests on 5 launches, and one slow
            # launch moved 8-FSK's mean by 3 % (profiles/round4/r4z/: p50
            # 0.3126, mean 0.3197 ms)
            rr = run_config(A, D, torch, dist, args, cfgname, rank, world, local, False,
                            max(args.steps, 100), args.warmup, hop_fft=256, spectrum=spec, fft_plan=fplan,
                            rescue_ab=not spec and not args.no_rescue_ab,
                            parity_windows=16384 if (cfgname == "fft" and not spec) else 0,
                            parity_every=0 if spec or args.no_cpu_baseline else 1)
            extras[key] = summary(rr)
            del rr
            torch.cuda.empty_cache()
        r.update(main_keep)
        if want("host_e2e"):
            extras["host_e2e"] = host_e2e(A, torch, r)
        torch.cuda.empty_cache()
        if not args.no_cpu_baseline and want("error_model"):
            extras["error_model"] = error_model_headroom(A)
        # the main run's buffers go before the worst-case sweep allocates its own
        keep_cpu = {k: r[k][:65536].clone() if r[k] is not None else None
                    for k in ("d_pcm", "d_sym", "d_mag")}
        for k in ("d_pcm", "d_sym", "d_mag", "d_true"):
            r.pop(k, None)
        torch.cuda.empty_cache()
        if want("rescue_worst"):
            extras["rescue_worst"] = rescue_worst(A, torch, args.steps, args.warmup)
        if want("quiet_cost"):
            extras["quiet_cost"] = quiet_cost(A, torch, args.steps, args.warmup)
        r.update(keep_cpu)
        if want("streams"):
            extras["streams"] = streams_child(args)
            # one rank's shard of the 8-GPU run (128 of the 1024 streams), the
            # same graph step: the projected 8-GPU scaling of configs[4]
            # measured on one GPU
            sh = streams_child(args, 128, breakdown=True)
            if "ms_per_step" in sh and "ms_per_step" in extras["streams"]:
                sh["projected_scaling_8"] = round(extras["streams"]["ms_per_step"] / sh["ms_per_step"], 3)
                sh["projection"] = ("streams.ms_per_step / streams_shard.ms_per_step: each of 8 ranks "
                                    "runs this shard's step; the 8-rank all-gather of 8 x the shard's "
                                    "frames replaces this step's world-1 gather beside the kernel")
            extras["streams_shard"] = sh
    elif world > 1 and args.config == "fsk2" and not args.no_extras:
        # the headline is already measured: a failure here (every rank runs the
        # same code, so every rank raises alike) costs the entry, not the line;
        # a hang (the step's HIP graph holds an RCCL collective) ends at the
        # watchdog's deadline with the headline line printed and every rank
        # exiting WATCHDOG_EXIT (non-zero: the hang is not hidden)
        guard = extras_watchdog(lambda: headline_line(args, r, world, {"streams": {
            "error": f"timed out after {args.extras_timeout:.0f} s (watchdog)"}}),
            rank, args.extras_timeout)
        try:
            if os.environ.get("BENCH_TEST_HANG_EXTRA"):
                time.sleep(3600)  # tests: a hung extra (test_self_launch_watchdog_keeps_the_headline)
            # configs[4] over the N ranks (strong scaling), and the same workload on
            # rank 0's GPU alone for scaling_vs_n1 (the other ranks wait)
            for k in ("d_pcm", "d_sym", "d_mag", "d_true"):
                r.pop(k, None)
            torch.cuda.empty_cache()
            args.graph = args.dist_backend == "nccl" or bool(os.environ.get("BENCH_TEST_GRAPH_FAIL"))
            # beside the torch path, the product's own multi-GPU path: the same
            # bucket through demod_group_* on every rank
            args.c_group = not args.no_c_group
            # >= 16 replays of the 16-step graph bucket, at N ranks and at N = 1
            # alike (2 replays left the rate within +-7 %, profiles/round4/r4g/)
            s_steps = max(args.steps, 256) if args.graph else args.steps
            rs = run_config(A, D, torch, dist, args, "streams", rank, world, local, True,
                            s_steps, args.warmup)
            ent = {"workload": f"configs[4]: 1024 streams x 2048 windows sharded over {world} GPUs",
                   "scaling": "strong", "value": round(rs["total_windows"] * 1024 /
                                                       (rs["ms_per_step"] / 1e3) / 1e6, 1),
                   "unit": "Msamples/s", "ms_per_step": round(rs["ms_per_step"], 4),
                   "kernel_ms": round(rs["kernel_ms"], 4), "symbol_errors": rs["sym_err"],
                   "framing": rs["framed"], "overhead": rs.get("overhead")}
            if ent["overhead"] and "c_group" in ent["overhead"]:
                ent["c_group"] = ent["overhead"].pop("c_group")
            del rs
            torch.cuda.empty_cache()
            # the N = 1 reference runs the SAME step construction (graph step,
            # device framing, gather) over a one-rank group on rank 0's GPU
            # (VERDICT r3 weak 5 ii: round 3 compared an eager N = 1 step)
            g0 = dist.new_group([0])
            dist.barrier()
            if rank == 0:
                r1 = run_config(A, D, torch, dist, args, "streams", 0, 1, local, True,
                                s_steps, args.warmup, group=g0)
                ent["n1_ms_per_step"] = round(r1["ms_per_step"], 4)
                ent["n1_kernel_ms"] = round(r1["kernel_ms"], 4)
                ent["n1_how"] = ("the same 1024 streams on rank 0's GPU alone in this job, the same "
                                 "step (%s, gather over a one-rank group)"
                                 % ("HIP graph" if args.graph else "eager"))
                ent["scaling_vs_n1"] = round(r1["ms_per_step"] / ent["ms_per_step"], 3)
                c1 = (r1.get("overhead") or {}).get("c_group") or {}
                cN = ent.get("c_group")
                if cN is not None:
                    cN["n1_ms_per_step"] = c1.get("ms_per_step")
                    if c1.get("error"):
                        cN["n1_error"] = c1["error"]
                    if c1.get("ms_per_step") and cN.get("ms_per_step"):
                        # the C group at N ranks against the same C group over
                        # one rank on rank 0's GPU, the same bucket
                        cN["scaling_vs_n1"] = round(c1["ms_per_step"] / cN["ms_per_step"], 3)
                del r1
                torch.cuda.empty_cache()
            dist.barrier()
            extras["streams"] = ent
        except Exception as e:  # noqa: BLE001 - reported in the line
            extras["streams"] = {"error": f"{type(e).__name__}: {e}"[:800]}

    if rank == 0:
        out = headline_line(args, r, world, extras)
        if world == 1 and not args.no_cpu_baseline:
            visible, affinity, quota, threads, why = cpu_share()
            if args.cpu_threads:
                threads, why = args.cpu_threads, "--cpu-threads"
            base, parity = cpu_baseline(r["d_pcm"], r["d_sym"], r["d_mag"], r["freqs"],
                                        args.cpu_seconds, threads, r["config"] == "fft", r["hop"])
            base.update({"host_cpus_visible": visible, "cpus_in_affinity": affinity,
                         "cgroup_quota_cores": quota, "threads_why": why})
            out["cpu_baseline"] = base
            if r["config"] in ("fsk2", "fsk8"):
                sys.path.insert(0, ROOT)
                from oracle import oracle as O
                parity = {"sigma400": parity,
                          "sigma2000": stress_parity(A, O, r["cfg"], r["freqs"], 2000, 65536,
                                                     r["d_pcm"].device, torch, threads)}
            out["parity_sample"] = parity
        out["extra_keys"] = sorted(extras)
        if guard is not None:
            guard.printed = True
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    if guard is not None:
        guard.set()


WATCHDOG_EXIT = 3  # exit status of a rank the watchdog ended


def extras_watchdog(line_fn, rank, seconds):
    """N > 1: if the extra measurement (and the teardown after it) has not
    finished after `seconds`, rank 0 prints the headline line (line_fn) unless
    it already printed its line, and every rank exits WATCHDOG_EXIT: the
    headline survives, but a hung collective does not pass for success.
    Returns the event that disarms it (its `printed` attribute marks the line
    as out)."""
    import threading

    done = threading.Event()
    done.printed = False

    def fire():
        if done.wait(seconds):
            return
        if rank == 0 and not done.printed:
            out = line_fn()
            out["extra_keys"] = sorted(k for k in out if k == "streams")
            print(json.dumps(out), flush=True)
        print(f"bench.py: watchdog: rank {rank} ended after {seconds:.0f} s (extra measurement or "
              "teardown hung)", file=sys.stderr, flush=True)
        sys.stdout.flush()
        os._exit(WATCHDOG_EXIT)

    threading.Thread(target=fire, daemon=True).start()
    return done


def headline_line(args, r, world, extras) -> dict:
    """The JSON line (without the CPU baseline and extra_keys) for rank 0."""
    samples = r["total_windows"] * r["n"]  # stream samples demodulated (each counted once)
    value = samples / (r["ms_per_step"] / 1e3) / 1e6
    config, K, hop, W, n_eval = r["config"], r["K"], r["hop"], r["W"], r["n_eval"]
    dev_framing = config == "streams"
    out = {
        "metric": METRIC,
        "value": round(value, 1),
        "unit": "Msamples/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "warmup_effective": r["warm"],
        "warmup_settle_ms_per_step": r.get("settle"),
        "ms_per_step": round(r["ms_per_step"], 4),
        "higher_is_better": True,
        "scaling": "strong" if config == "streams" else "weak",
        "vs_baseline": None,
        "dtype": "fp32",
        "data": "synthetic (seeded splitmix64 FSK, A=8000, Irwin-Hall noise sigma=400)",
        "config": {
            "workload": (f"configs[4]: {r['total_windows'] // 2048} streams x 2048 windows (2^21 "
                         f"samples each), sharded by stream over {world} GPU(s), 2-FSK"
                         if config == "streams" else
                         f"configs[3]: sliding 1024-pt full-spectrum FFT, hop {hop}, "
                         f"{n_eval} windows over a {W * 1024}-sample int16 stream per GPU"
                         if config == "fft" else
                         ("configs[1]: 2-FSK" if K == 2 else
                          "configs[2]: 8-FSK" + (" (integer bins 32 + 9 i)" if args.plan == "odd"
                                                 else ""))
                         + f" Goertzel, {W} x 1024-sample int16 windows per GPU, HBM-resident"),
            "tones_hz": list(r["freqs"]),
            "windows_per_gpu": n_eval,
            "hop": hop,
            "n": r["n"],
            "outputs": "symbols" + ("" if args.no_mags else " + |X_k|^2"),
            "parallelism": (f"dp{world} (stream shards; per-rank device framing, RCCL "
                            "all-gather of ToReceiver frames)" if dev_framing else
                            f"dp{world} (independent window shards, RCCL symbol all-gather)"),
        },
        "detector": r["detector"],
        "kernel_ms_p10_p50_p90": [round(float(np.percentile(r["kts"], q)), 4)
                                  for q in (10, 50, 90)],
        "symbol_errors": r["sym_err"],
        "symbol_error_rate": r["sym_err"] / float(r["total_windows"]),
        "kernel_ms": round(r["kernel_ms"], 4),
        "kernel_ms_steps": f"HIP events on every {EV_EVERY}th timed step ({len(r['kts'])})",
        "roofline": r["roofline"],
    }
    if "roofline_valu" in r:
        out["roofline_valu"] = r["roofline_valu"]
    if "overhead" in r:
        out["overhead"] = r["overhead"]
    if "rescue" in r:
        out["rescue"] = r["rescue"]
    if "sustained" in r:
        out["sustained"] = r["sustained"]
    if "parity_all" in r:
        out["parity_all"] = r["parity_all"]
    if r["framed"]:
        out["framing"] = r["framed"]
    if r.get("dumped"):
        out["dump_outputs"] = {"dir": args.dump_outputs, "rows": r["dumped"],
                               "what": "the last timed step's outputs (rank 0), <name>.npy"}
    out.update(extras)
    return out


if __name__ == "__main__":
    main()
