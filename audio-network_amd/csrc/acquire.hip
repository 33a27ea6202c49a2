// acquire.hip — symbol timing and sync-word acquisition over a detector
// batch's outputs (include/demod.h "acquisition").
//
// Inputs: sym[W] and P[W][K] of W sliding windows (window w at sample w hop),
// R = n / hop phases. Three launches on the caller's stream:
//
//  scan      a fixed-size grid walks tiles of kAcqTile windows (block b takes
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
#include "../../include/demod.h"
#include "demod_internal.h"

namespace fskd {

constexpr int kAcqThreads = 256;
constexpr int kAcqPerThread = kAcqTile / kAcqThreads;
constexpr int kAcqHalo = (DEMOD_MAX_SYNC - 1) * DEMOD_MAX_PHASES;
constexpr unsigned long long kAcqNone = ~0ull;

static_assert(kAcqTile % kAcqThreads == 0 && kAcqThreads % DEMOD_MAX_PHASES == 0,
              "a thread's windows must stay on one phase");

__global__ __launch_bounds__(kAcqThreads) void acquire_scan_kernel(AcquireParams p)
{
    __shared__ uint8_t s_sym[kAcqTile + kAcqHalo];
    __shared__ uint8_t s_sync[DEMOD_MAX_SYNC];
    __shared__ unsigned long long s_first[DEMOD_MAX_PHASES];
    __shared__ double s_acc[kAcqThreads];
    const int t = threadIdx.x, R = p.phases, L = p.sync_len;
    const long long W = p.n_windows, Wm = p.per_phase * R;
    const int halo = L > 0 ? (L - 1) * R : 0;
    if (t < DEMOD_MAX_PHASES) s_first[t] = kAcqNone;
    if (t < DEMOD_MAX_SYNC) s_sync[t] = p.sync[t];
    double acc = 0.0;
    const long long tiles = (W + kAcqTile - 1) / kAcqTile;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long base = tile * kAcqTile;
        __syncthreads();  // the previous tile's compares have read s_sym
        uint8_t sv[kAcqPerThread];
#pragma unroll
        for (int i = 0; i < kAcqPerThread; ++i) {
            const long long w = base + t + kAcqThreads * i;
            sv[i] = w < W ? p.sym[w] : (uint8_t)0xFF;
            s_sym[t + kAcqThreads * i] = sv[i];
        }
        for (int h = t; h < halo; h += kAcqThreads) {
            const long long w = base + kAcqTile + h;
            s_sym[kAcqTile + h] = w < W ? p.sym[w] : (uint8_t)0xFF;
        }
        // the decided tone's power; a byte >= K reads nothing and adds nothing
        float pw[kAcqPerThread];
#pragma unroll
        for (int i = 0; i < kAcqPerThread; ++i) {
            const long long w = base + t + kAcqThreads * i;
            pw[i] = (w < Wm && sv[i] < p.k) ? p.mag[w * p.k + sv[i]] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kAcqPerThread; ++i) acc += (double)pw[i];
        __syncthreads();
        if (L > 0) {
#pragma unroll 1
            for (int i = 0; i < kAcqPerThread; ++i) {
                const int local = t + kAcqThreads * i;
                const long long w = base + local;
                if (w + halo >= W) continue;  // the word would run past the batch
                unsigned err = 0;
                for (int j = 0; j < L; ++j) {
                    err += s_sym[local + j * R] != s_sync[j];
                    if (err > p.max_errors) break;
                }
                if (err <= p.max_errors)
                    atomicMin(&s_first[local & (R - 1)], ((unsigned long long)w << 8) | err);
            }
        }
    }
    s_acc[t] = acc;
    __syncthreads();
    if (t < R) {
        double m = 0.0;
#pragma unroll 8
        for (int g = t; g < kAcqThreads; g += R) m += s_acc[g];
        p.part[(long long)blockIdx.x * R + t] = m;
        p.first[(long long)blockIdx.x * R + t] = s_first[t];
    }
}

__global__ __launch_bounds__(kAcqThreads) void acquire_final_kernel(AcquireParams p)
{
    __shared__ double s_m[DEMOD_MAX_PHASES];
    __shared__ double s_acc[kAcqThreads];
    __shared__ unsigned long long s_best;
    __shared__ int s_phase;
    const int t = threadIdx.x, R = p.phases;
    demod_acquire_result_t *res = p.res;
    // the partials [grid][R] as one array: entry i is on phase i mod R and 256
    // is a multiple of R, so thread t adds entries t, t + 256, .. (coalesced,
    // in block order), then thread r adds the threads' sums of its phase in
    // thread order: the scan's own scheme, short chains of adds in a fixed order
    const long long total = (long long)p.grid * R;
    double m = 0.0;
#pragma unroll 4
    for (long long i = t; i < total; i += kAcqThreads) m += p.part[i];
    s_acc[t] = m;
    __syncthreads();
    if (t < DEMOD_MAX_PHASES) {
        double v = 0.0;
        if (t < R) {
#pragma unroll 8
            for (int g = t; g < kAcqThreads; g += R) v += s_acc[g];
        }
        s_m[t] = v;          // 0 for t >= R
        res->metric[t] = v;
    }
    if (t == 0) s_best = kAcqNone;
    __syncthreads();
    if (t == 0) {
        int best = 0;
        for (int r = 1; r < R; ++r)
            if (s_m[r] > s_m[best]) best = r;
        s_phase = best;
    }
    __syncthreads();
    const int phase = s_phase;
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
