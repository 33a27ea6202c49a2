// acquire_scan.h — the scan that acquire.hip and acquire_frames.hip share: one
// copy of the thread-to-window map, the order of the phase sums, the LDS
// staging of a tile's symbols and the sync-word compare, so the two kernels
// cannot drift. Their phase metrics are bit-identical on the same inputs
// because both run this body over the same grid (acquire_grid).
//
// A fixed-size grid walks tiles of kAcqTile windows (block b takes tiles b,
// b + grid, ..). Thread t owns the tile's windows t + 256 i: 256 and the tile
// are multiples of R, so every window a thread ever sees is on phase t mod R
// and the thread carries ONE double sum of the decided tone's power, in window
// order. The tile's symbols and the (sync_len - 1) R that follow it are staged
// in LDS once (0xFF past the batch's end); every start of the tile whose word
// fits the batch is compared against LDS (stride R, leaving at the first error
// past max_errors). What becomes of a match is the caller's: on_hit(local, w,
// errors) is called for each, tile_done(tile) by every thread once the tile's
// compares are issued (it may hold barriers: every thread of the block calls
// it the same number of times). At the end the block adds its threads' sums
// per phase in thread order and stores one partial per phase to part[block][R]
// by plain stores.
#pragma once
#include "../../include/demod.h"
#include "demod_internal.h"

namespace fskd {

constexpr int kAcqThreads = 256;
constexpr int kAcqPerThread = kAcqTile / kAcqThreads;
constexpr int kAcqHalo = (DEMOD_MAX_SYNC - 1) * DEMOD_MAX_PHASES;
constexpr unsigned long long kAcqNone = ~0ull;

static_assert(kAcqTile % kAcqThreads == 0 && kAcqThreads % DEMOD_MAX_PHASES == 0,
              "a thread's windows must stay on one phase");

// What the scan reads: the fields AcquireParams and FramesParams have in common.
struct AcqScanArgs {
    const uint8_t *sym;      // [n_windows]
    const float *mag;        // [n_windows][k]
    long long n_windows;
    long long per_phase;     // J = n_windows / phases
    int phases;              // R
    int k;
    int sync_len;
    unsigned max_errors;
    double *part;            // [grid][phases]
};

struct AcqScanLds {
    uint8_t sym[kAcqTile + kAcqHalo];
    uint8_t sync[DEMOD_MAX_SYNC];
    double acc[kAcqThreads];
};

// errors of the word at the tile-local start `local`, or a count above
// max_errors as soon as it is passed
__device__ __forceinline__ unsigned acq_word_errors(const uint8_t *s_sym, const uint8_t *s_sync,
                                                    int local, int R, int L, unsigned max_errors)
{
    unsigned err = 0;
    for (int j = 0; j < L; ++j) {
        err += s_sym[local + j * R] != s_sync[j];
        if (err > max_errors) break;
    }
    return err;
}

// the tile's symbols and halo into LDS; sv: this thread's own kAcqPerThread
__device__ __forceinline__ void acq_stage_tile(const uint8_t *sym, long long W, long long base,
                                               int halo, uint8_t *s_sym, uint8_t (&sv)[kAcqPerThread])
{
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < kAcqPerThread; ++i) {
        const long long w = base + t + kAcqThreads * i;
        sv[i] = w < W ? sym[w] : (uint8_t)0xFF;
        s_sym[t + kAcqThreads * i] = sv[i];
    }
    for (int h = t; h < halo; h += kAcqThreads) {
        const long long w = base + kAcqTile + h;
        s_sym[kAcqTile + h] = w < W ? sym[w] : (uint8_t)0xFF;
    }
}

template <typename OnHit, typename TileDone>
__device__ __forceinline__ void acquire_scan_body(const AcqScanArgs &p, const uint8_t *sync,
                                                  AcqScanLds &s, OnHit &&on_hit, TileDone &&tile_done)
{
    const int t = threadIdx.x, R = p.phases, L = p.sync_len;
    const long long W = p.n_windows, Wm = p.per_phase * R;
    const int halo = L > 0 ? (L - 1) * R : 0;
    if (t < DEMOD_MAX_SYNC) s.sync[t] = sync[t];
    double acc = 0.0;
    const long long tiles = (W + kAcqTile - 1) / kAcqTile;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long base = tile * kAcqTile;
        __syncthreads();  // the previous tile's compares have read s.sym
        uint8_t sv[kAcqPerThread];
        acq_stage_tile(p.sym, W, base, halo, s.sym, sv);
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
                const unsigned err = acq_word_errors(s.sym, s.sync, local, R, L, p.max_errors);
                if (err <= p.max_errors) on_hit(local, w, err);
            }
        }
        tile_done(tile);
    }
    s.acc[t] = acc;
    __syncthreads();
    if (t < R) {
        double m = 0.0;
#pragma unroll 8
        for (int g = t; g < kAcqThreads; g += R) m += s.acc[g];
        p.part[(long long)blockIdx.x * R + t] = m;
    }
}

// The finaliser's first half, by one workgroup of kAcqThreads: the partials
// [grid][R] as one array. Entry i is on phase i mod R and 256 is a multiple of
// R, so thread t adds entries t, t + 256, .. (coalesced, in block order), then
// thread r adds the threads' sums of its phase in thread order: the scan's own
// scheme, short chains of adds in a fixed order. metric[r] (0 for r >= R) is
// stored, and the argmax with ties to the lowest phase is returned to every
// thread. s_acc: kAcqThreads doubles, s_m: DEMOD_MAX_PHASES, s_phase: one int.
__device__ __forceinline__ int acquire_final_phase(const double *part, int grid, int R, double *metric,
                                                   double *s_acc, double *s_m, int *s_phase)
{
    const int t = threadIdx.x;
    const long long total = (long long)grid * R;
    double m = 0.0;
#pragma unroll 4
    for (long long i = t; i < total; i += kAcqThreads) m += part[i];
    s_acc[t] = m;
    __syncthreads();
    if (t < DEMOD_MAX_PHASES) {
        double v = 0.0;
        if (t < R) {
#pragma unroll 8
            for (int g = t; g < kAcqThreads; g += R) v += s_acc[g];
        }
        s_m[t] = v;          // 0 for t >= R
        metric[t] = v;
    }
    __syncthreads();
    if (t == 0) {
        int best = 0;
        for (int r = 1; r < R; ++r)
            if (s_m[r] > s_m[best]) best = r;
        *s_phase = best;
    }
    __syncthreads();
    return *s_phase;
}

}  // namespace fskd
