// acquire_seg_scan.h — what acquire_segments.hip and acquire_frames_segments.hip
// share: one copy of the tile lookup, the lane-to-window map, the staging of a
// tile's symbols in the wave's LDS slab (0xFF past the segment's end), the
// order of the phase sums, the butterfly over the lanes of a phase, the
// sync-word compare and the finaliser's phase decision, so the two cannot
// drift. Their phase metrics are bit-identical on the same tables because both
// run these bodies over the same plan (acquire_seg_plan_kernel's header).
//
// A tile is kAcqTile segment-relative windows taken by ONE WAVE; lane l owns
// windows l + 64 i, all on phase l mod R. What a match does differs between
// the two (seg_scan_tile's kFrames): the acquisition keeps the lowest one, the
// frame scan counts the complete ones and keeps the lowest incomplete one.
#pragma once
#include "acquire_scan.h"

namespace fskd {

constexpr int kSegThreads = 256;
constexpr int kSegLanes = 64;
constexpr int kSegWaves = kSegThreads / kSegLanes;
constexpr int kSegPerLane = kAcqTile / kSegLanes;
constexpr int kSegHalo = (DEMOD_MAX_SYNC - 1) * DEMOD_MAX_PHASES;
constexpr int kSegMaxBlocks = 2048;      // the scan's grid: min(ceil(budget / 4), this)
constexpr unsigned kSegWaveTiles = 64;   // finalise: up to this many tiles by one wave
constexpr unsigned long long kSegNone = ~0ull;

static_assert(kSegLanes % DEMOD_MAX_PHASES == 0 && kAcqTile % kSegLanes == 0,
              "a lane's windows must stay on one phase");
static_assert(kSegThreads % DEMOD_MAX_PHASES == 0, "finalise: a thread's entries stay on one phase");

// the grid of a launch whose waves walk the call's tiles
inline unsigned seg_tile_grid(unsigned budget)
{
    const unsigned long long blocks = ((unsigned long long)budget + kSegWaves - 1) / kSegWaves;
    return (unsigned)(blocks < kSegMaxBlocks ? (blocks ? blocks : 1) : kSegMaxBlocks);
}

// Tile g of the call: its segment, the segment's clamped table entry and the
// tile's first window relative to the segment. All zero for g >= total.
struct SegTile {
    bool live;
    unsigned s;
    long long cnt;              // count'
    unsigned long long f;       // first'
    long long base;
};

__device__ __forceinline__ SegTile seg_tile_of(const AcquireSegParams &p, unsigned g, unsigned total)
{
    SegTile tl;
    tl.live = g < total;
    // the last segment whose first tile is <= g: zero-tile segments share a
    // successor's first tile and lie before it, dropped ones start at total
    unsigned s = 0;
    if (tl.live) {
        unsigned lo = 0, hi = p.n_segments;
        while (hi - lo > 1) {
            const unsigned mid = lo + (hi - lo) / 2;
            if (p.w_tile0[mid] <= g) lo = mid; else hi = mid;
        }
        s = lo;
    }
    tl.s = s;
    tl.cnt = tl.live ? (long long)p.w_count[s] : 0;
    tl.f = tl.live ? p.w_first[s] : 0;
    tl.base = tl.live ? (long long)(g - p.w_tile0[s]) * kAcqTile : 0;
    return tl;
}

// the tile's symbols (sv: this lane's own) and, with to_lds, the tile and the
// `halo` symbols after it into the wave's slab. (tl by value here and below:
// by reference the segment's base address is recomputed at every load.)
__device__ __forceinline__ void seg_stage_tile(const AcquireSegParams &p, const SegTile tl, int halo,
                                               uint8_t *slab, int lane, bool to_lds,
                                               uint8_t (&sv)[kSegPerLane])
{
    // Every load is issued whatever the window (at an index clamped into the
    // segment) and the value selected afterwards: the loads of a lane do not
    // wait for each other. A tile past the call's total has no segment to read.
    const uint8_t *sym = p.sym + tl.f;   // the segment's first symbol
    const long long last = tl.cnt - 1;
#pragma unroll
    for (int i = 0; i < kSegPerLane; ++i) sv[i] = 0xFF;
    if (tl.cnt > 0) {
#pragma unroll
        for (int i = 0; i < kSegPerLane; ++i) {
            const long long w = tl.base + lane + kSegLanes * i;
            const uint8_t v = sym[w < tl.cnt ? w : last];
            sv[i] = w < tl.cnt ? v : (uint8_t)0xFF;
        }
    }
    if (to_lds) {
#pragma unroll
        for (int i = 0; i < kSegPerLane; ++i) slab[lane + kSegLanes * i] = sv[i];
    }
    for (int h = lane; h < halo; h += kSegLanes) {
        const long long w = tl.base + kAcqTile + h;
        slab[kAcqTile + h] = w < tl.cnt ? sym[w] : (uint8_t)0xFF;
    }
}

// One tile by one wave (every thread of the workgroup calls it the same number
// of times: it holds barriers). acc is the tile's phase sum, word and count what
// the sync-word compare found, each the same value in every lane of a phase:
//   kFrames false  word is the lowest match (w << 8 | errors) of the phase,
//                  kSegNone without one: a lane's windows ascend, so its first
//                  match is its lowest and ends its compares. count is 0.
//   kFrames true   a match at w is complete when w + span < count' (its word
//                  and payload fit the segment) and is counted; word is the
//                  phase's lowest match that is not complete: every later start
//                  of the lane is incomplete too, so it ends the lane's compares.
// Both go through the same xor butterfly as the sum (integer add, integer min).
struct SegScan {
    double acc;
    unsigned long long word;
    unsigned count;
};

template <bool kFrames>
__device__ __forceinline__ SegScan seg_scan_tile(const AcquireSegParams &p, const SegTile tl, uint8_t *slab,
                                                 const uint8_t *s_sync, int lane, long long span)
{
    const int R = p.phases, L = p.sync_len;
    const int halo = L > 0 ? (L - 1) * R : 0;
    const long long cnt = tl.cnt, base = tl.base;
    const unsigned long long f = tl.f;
    const long long Wm = cnt / R * R;
    if (L > 0) __syncthreads();  // the previous tile's compares have read the slab
    uint8_t sv[kSegPerLane];
    seg_stage_tile(p, tl, halo, slab, lane, L > 0, sv);
    // the decided tone's power; a byte >= K reads nothing and adds nothing
    // (loaded whatever the window, from the segment's first row where it does
    // not count, and selected afterwards, as the symbols are)
    const float *mag = p.mag + f * p.k;   // the segment's first row
    float pw[kSegPerLane];
#pragma unroll
    for (int i = 0; i < kSegPerLane; ++i) pw[i] = 0.f;
    if (Wm > 0) {
#pragma unroll
        for (int i = 0; i < kSegPerLane; ++i) {
            const long long w = base + lane + kSegLanes * i;
            const bool in = w < Wm && sv[i] < p.k;
            const float v = mag[in ? w * p.k + sv[i] : 0];
            pw[i] = in ? v : 0.f;
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < kSegPerLane; ++i) acc += (double)pw[i];
    unsigned long long word = kSegNone;
    unsigned count = 0;
    if (L > 0) {
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < kSegPerLane; ++i) {
            const int local = lane + kSegLanes * i;
            const long long w = base + local;
            if (w + halo >= cnt) break;  // the word would run past the segment
            unsigned err = 0;
            for (int j = 0; j < L; ++j) {
                err += slab[local + j * R] != s_sync[j];
                if (err > p.max_errors) break;
            }
            if (err <= p.max_errors) {
                if (kFrames && w + span < cnt) {
                    ++count;
                } else {
                    word = ((unsigned long long)w << 8) | err;
                    break;
                }
            }
        }
    }
    // the lanes of a phase: a fixed tree, the same value in every lane of it
    for (int off = kSegLanes / 2; off >= R; off >>= 1) {
        acc += __shfl_xor(acc, off);
        const unsigned long long o = __shfl_xor(word, off);
        word = o < word ? o : word;
        if (kFrames) count += __shfl_xor(count, off);
    }
    return {acc, word, count};
}

// The finaliser's first half, by a workgroup of kSegThreads whose wave v takes
// segment 4 blockIdx.x + v: the segment's partials [tiles][R] read as one
// array, lane l adding entries l, l + 64, .., then the butterfly; segments of
// more than kSegWaveTiles tiles are added by the whole workgroup instead
// (thread t entries t, t + 256, .., then thread r its phase's threads in order,
// as acquire_final_kernel). Argmax with ties to the lowest phase, then the
// lowest of the chosen phase's words p.first[tile][phase] (kSegNone: none; not
// read when sync_len == 0). Every thread of the workgroup calls it.
struct SegFinalLds {
    double acc[kSegThreads];
    double big[kSegWaves][DEMOD_MAX_PHASES];
    unsigned nt[kSegWaves], t0[kSegWaves];
    unsigned long long best[kSegWaves];
    int phase[kSegWaves];
};

struct SegFinal {
    bool valid;                 // s < n_segments
    unsigned s, nt, t0;         // nt == 0: a short segment
    unsigned long long cnt;     // count'
    double m;                   // lane l: the metric of phase l mod R
    int phase;
    unsigned long long best;
};

__device__ __forceinline__ SegFinal seg_final_phase(const AcquireSegParams &p, SegFinalLds &l)
{
    const int t = threadIdx.x, wave = t / kSegLanes, lane = t % kSegLanes, R = p.phases;
    SegFinal r;
    r.s = blockIdx.x * kSegWaves + wave;
    r.valid = r.s < p.n_segments;
    const unsigned nt = r.valid ? p.w_tiles[r.s] : 0u;
    const unsigned t0 = r.valid ? p.w_tile0[r.s] : 0u;
    r.nt = nt;
    r.t0 = t0;
    r.cnt = r.valid ? p.w_count[r.s] : 0u;
    if (lane == 0) {
        l.nt[wave] = nt;
        l.t0[wave] = t0;
        l.best[wave] = kSegNone;
    }
    __syncthreads();
    double m = 0.0;   // lane l: the metric of phase l mod R
    if (nt <= kSegWaveTiles) {
        const double *q = p.part + (size_t)t0 * R;
        const unsigned total = nt * (unsigned)R;
#pragma unroll 4
        for (unsigned i = lane; i < total; i += kSegLanes) m += q[i];
        for (int off = kSegLanes / 2; off >= R; off >>= 1) m += __shfl_xor(m, off);
    }
    // long segments: the whole workgroup, one after the other (uniform branches)
    for (int w = 0; w < kSegWaves; ++w) {
        const unsigned ntw = l.nt[w];
        if (ntw <= kSegWaveTiles) continue;
        const double *q = p.part + (size_t)l.t0[w] * R;
        const unsigned long long total = (unsigned long long)ntw * R;
        double a = 0.0;
#pragma unroll 8
        for (unsigned long long i = t; i < total; i += kSegThreads) a += q[i];
        l.acc[t] = a;
        __syncthreads();
        if (t < R) {
            double v = 0.0;
#pragma unroll 8
            for (int g = t; g < kSegThreads; g += R) v += l.acc[g];
            l.big[w][t] = v;
        }
        __syncthreads();
        // its phase and that phase's lowest word, by the workgroup too: one
        // wave would wait for tiles / 64 loads one after the other
        if (t == 0) {
            int best = 0;
            for (int r2 = 1; r2 < R; ++r2)
                if (l.big[w][r2] > l.big[w][best]) best = r2;
            l.phase[w] = best;
        }
        __syncthreads();
        if (p.sync_len > 0) {
            const unsigned long long *f = p.first + (size_t)l.t0[w] * R + l.phase[w];
            unsigned long long v = kSegNone;
#pragma unroll 4
            for (unsigned b = t; b < ntw; b += kSegThreads) {
                const unsigned long long o = f[(size_t)b * R];
                v = o < v ? o : v;
            }
            if (v != kSegNone) atomicMin(&l.best[w], v);   // integer, LDS
        }
        __syncthreads();
    }
    if (nt > kSegWaveTiles) m = l.big[wave][lane & (R - 1)];
    // argmax over the phases, ties to the lowest
    double bm = m;
    int br = lane & (R - 1);
    for (int off = R >> 1; off >= 1; off >>= 1) {
        const double om = __shfl_xor(bm, off);
        const int orr = __shfl_xor(br, off);
        if (om > bm || (om == bm && orr < br)) {
            bm = om;
            br = orr;
        }
    }
    const int phase = nt > kSegWaveTiles ? l.phase[wave] : __shfl(br, 0);
    unsigned long long best = nt > kSegWaveTiles ? l.best[wave] : kSegNone;
    if (p.sync_len > 0 && nt <= kSegWaveTiles) {
        for (unsigned b = lane; b < nt; b += kSegLanes) {
            const unsigned long long v = p.first[((size_t)t0 + b) * R + phase];
            best = v < best ? v : best;
        }
        for (int off = kSegLanes / 2; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off);
            best = o < best ? o : best;
        }
    }
    r.m = m;
    r.phase = phase;
    r.best = best;
    return r;
}

}  // namespace fskd
