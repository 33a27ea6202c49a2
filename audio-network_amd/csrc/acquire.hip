// acquire.hip — symbol timing and sync-word acquisition over a detector
// batch's outputs (include/demod.h "acquisition").
//
// Inputs: sym[W] and P[W][K] of W sliding windows (window w at sample w hop),
// R = n / hop phases. Three launches on the caller's stream:
//
//  scan      (its body is acquire_scan.h's, which acquire_frames.hip runs too)
//            a fixed-size grid walks tiles of kAcqTile windows (block b takes
//            tiles b, b + grid, ..). Thread t owns the tile's windows t + 256 i:
//            256 and the tile are multiples of R (a power of two, as n and hop
//            are), so every window a thread ever sees is on phase t mod R and
//            the thread carries ONE double sum of the decided tone's power, in
//            window order. The tile's symbols and the (sync_len - 1) R that
//            follow it are staged in LDS once; every legal start of the tile
//            compares the sync word against LDS (stride R, leaving at the
//            first error past max_errors) and a match lowers its phase's
//            (w << 8 | errors) by an integer 64-bit atomicMin in LDS. At the
//            end the block sums its threads' sums per phase in thread order
//            and stores one partial and one first-match word per phase to
//            d_work: every word of d_work the next launch reads is stored
//            here by plain stores, so there is nothing to initialise and a
//            captured graph's replays start clean. No floating-point atomics:
//            the order of every sum is fixed by the shape alone.
//  finalise  one workgroup: the partials summed the same way (thread t takes
//            entries t, t + 256, .. of [grid][R] in block order, then thread r
//            its phase's threads in order), argmax with ties to the lowest phase, that phase's lowest first-match word over
//            the blocks, and every byte of *d_result.
//  gather    out[j] = sym[first_window + j R], j < n_written, both read from
//            *d_result (skipped when cap == 0).
#include "acquire_scan.h"

namespace fskd {

static __device__ __forceinline__ AcqScanArgs scan_args(const AcquireParams &p)
{
    return {p.sym, p.mag, p.n_windows, p.per_phase, p.phases, p.k, p.sync_len, p.max_errors, p.part};
}

// the scan itself is acquire_scan.h's (shared with acquire_frames.hip); here a
// match lowers its phase's first-match word
__global__ __launch_bounds__(kAcqThreads) void acquire_scan_kernel(AcquireParams p)
{
    __shared__ AcqScanLds s;
    __shared__ unsigned long long s_first[DEMOD_MAX_PHASES];
    const int t = threadIdx.x, R = p.phases;
    if (t < DEMOD_MAX_PHASES) s_first[t] = kAcqNone;
    acquire_scan_body(
        scan_args(p), p.sync, s,
        [&](int local, long long w, unsigned err) {
            atomicMin(&s_first[local & (R - 1)], ((unsigned long long)w << 8) | err);
        },
        [](long long) {});
    // (the body's last barrier stands between the atomics and this read)
    if (t < R) p.first[(long long)blockIdx.x * R + t] = s_first[t];
}

__global__ __launch_bounds__(kAcqThreads) void acquire_final_kernel(AcquireParams p)
{
    __shared__ double s_m[DEMOD_MAX_PHASES];
    __shared__ double s_acc[kAcqThreads];
    __shared__ unsigned long long s_best;
    __shared__ int s_phase;
    const int t = threadIdx.x, R = p.phases;
    demod_acquire_result_t *res = p.res;
    if (t == 0) s_best = kAcqNone;
    const int phase = acquire_final_phase(p.part, p.grid, R, res->metric, s_acc, s_m, &s_phase);
    if (p.sync_len > 0) {
        unsigned long long v = kAcqNone;
        for (int b = t; b < p.grid; b += kAcqThreads) {
            const unsigned long long f = p.first[(long long)b * R + phase];
            v = f < v ? f : v;
        }
        if (v != kAcqNone) atomicMin(&s_best, v);
    }
    __syncthreads();
    if (t == 0) {
        const unsigned long long W = (unsigned long long)p.n_windows;
        const bool found = p.sync_len > 0 && s_best != kAcqNone;
        unsigned long long fw = (unsigned long long)phase;
        if (p.sync_len > 0) fw = found ? (s_best >> 8) + (unsigned long long)p.sync_len * R : W;
        const unsigned long long n_out = fw < W ? (W - fw + R - 1) / R : 0;
        res->phases = (uint32_t)R;
        res->phase = (uint32_t)phase;
        res->per_phase = (uint64_t)p.per_phase;
        res->sync_window = found ? (int64_t)(s_best >> 8) : -1;
        res->sync_errors = found ? (uint32_t)(s_best & 0xFF) : 0u;
        res->reserved = 0;
        res->first_window = fw;
        res->n_out = n_out;
        res->n_written = n_out < p.cap ? n_out : p.cap;
    }
}

__global__ __launch_bounds__(kAcqThreads) void acquire_gather_kernel(AcquireParams p)
{
    const unsigned long long n = p.res->n_written, fw = p.res->first_window;
    const unsigned long long step = (unsigned long long)gridDim.x * kAcqThreads;
    for (unsigned long long j = (unsigned long long)blockIdx.x * kAcqThreads + threadIdx.x; j < n; j += step)
        p.out[j] = p.sym[fw + j * p.phases];
}

int acquire_grid(long long n_windows)
{
    const long long tiles = (n_windows + kAcqTile - 1) / kAcqTile;
    return (int)(tiles < kAcqMaxBlocks ? tiles : kAcqMaxBlocks);
}

hipError_t launch_acquire(AcquireParams p, hipStream_t s)
{
    p.grid = acquire_grid(p.n_windows);
    hipLaunchKernelGGL(acquire_scan_kernel, dim3(p.grid), dim3(kAcqThreads), 0, s, p);
    hipLaunchKernelGGL(acquire_final_kernel, dim3(1), dim3(kAcqThreads), 0, s, p);
    if (p.cap > 0) {
        const unsigned long long blocks = (p.cap + kAcqThreads - 1) / kAcqThreads;
        hipLaunchKernelGGL(acquire_gather_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)),
                           dim3(kAcqThreads), 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace fskd
