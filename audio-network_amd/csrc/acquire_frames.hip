// acquire_frames.hip — the frame scan (include/demod.h "frame scan", DESIGN.md
// §4.9 "Frames"): the phase decision of acquire.hip, then EVERY sync-word hit
// on that phase in ascending window order, each with a fixed-length payload as
// symbols and / or packed bytes. Four launches on the caller's stream whatever
// the hit count is (three without payload outputs, two when max_frames == 0):
//
//  scan      acquire_scan.h's body over acquire.hip's grid, so the phase sums
//            are bit-identical to demod_acquire_async's. The phase is not known
//            yet, so a match is kept for its own phase: a complete hit (word
//            and payload inside the batch) is counted, per tile and phase; an
//            incomplete one lowers its phase's (w << 8 | errors) by an integer
//            atomicMin in LDS. A thread's windows are all on one phase: it
//            counts in a register and adds once per tile to its phase's LDS
//            counter (integer, order-free). count[tile][R] and, per block,
//            tail[block][R] and part[block][R] go to d_work by plain stores.
//  finalise  one workgroup: partials, argmax and ties as acquire_final_kernel
//            (acquire_final_phase); the chosen phase's lowest tail word; the
//            exclusive prefix of that phase's column of count[][] into
//            offs[tiles] (thread t a contiguous chunk of ceil(tiles / 256),
//            then the 256 chunk totals through LDS); every byte of *d_result.
//  emit      per tile holding hits of the chosen phase (count[tile][phase] > 0
//            and offs[tile] < max_frames, both block-uniform): the tile staged
//            again, only the starts on the phase compared (start t + 256 i of
//            the tile's 1024 / R in round i), a hit's rank from the rounds
//            before, the waves before (totals through LDS) and the lanes
//            before (ballot, popcount below the lane): ascending w by
//            construction. hits[offs[tile] + rank] is stored when the index is
//            below max_frames. No atomics decide a position.
//  gather    reads n_written and the hits' windows from device memory:
//            payload[i N + j] = sym[w_i + (L + j) R], coalesced along j; and one
//            thread per packed byte, assembled from the symbols it spans, so no
//            two threads share a byte.
//
// Every word of d_work a launch reads was stored by an earlier launch of the
// same call. No floating-point atomics; every output byte is a function of the
// inputs alone.
#include "acquire_scan.h"
#include "frame_rows.h"

namespace fskd {

static __device__ __forceinline__ AcqScanArgs scan_args(const FramesParams &p)
{
    return {p.sym, p.mag, p.n_windows, p.per_phase, p.phases, p.k, p.sync_len, p.max_errors, p.part};
}

__global__ __launch_bounds__(kAcqThreads) void frames_scan_kernel(FramesParams p)
{
    __shared__ AcqScanLds s;
    __shared__ unsigned long long s_tail[DEMOD_MAX_PHASES];
    __shared__ unsigned s_cnt[DEMOD_MAX_PHASES];
    const int t = threadIdx.x, R = p.phases;
    const long long W = p.n_windows, span = frame_span(p.sync_len, p.frame_symbols, p.phases);
    if (t < DEMOD_MAX_PHASES) {
        s_tail[t] = kAcqNone;
        s_cnt[t] = 0;
    }
    unsigned mine = 0;   // this thread's complete hits of the tile, all on phase t mod R
    acquire_scan_body(
        scan_args(p), p.sync, s,
        [&](int local, long long w, unsigned err) {
            if (w + span < W)
                ++mine;
            else
                atomicMin(&s_tail[local & (R - 1)], ((unsigned long long)w << 8) | err);
        },
        [&](long long tile) {
            if (mine) atomicAdd(&s_cnt[t & (R - 1)], mine);   // integer, LDS
            mine = 0;
            __syncthreads();
            if (t < R) {
                p.count[tile * R + t] = s_cnt[t];
                s_cnt[t] = 0;   // the next tile adds after two more barriers
            }
        });
    // (the body's last barrier stands between the atomics and this read)
    if (t < R) p.tail[(long long)blockIdx.x * R + t] = s_tail[t];
}

__global__ __launch_bounds__(kAcqThreads) void frames_final_kernel(FramesParams p)
{
    __shared__ double s_m[DEMOD_MAX_PHASES];
    __shared__ double s_acc[kAcqThreads];
    __shared__ unsigned s_chunk[kAcqThreads];
    __shared__ unsigned long long s_best;
    __shared__ int s_phase;
    const int t = threadIdx.x, R = p.phases;
    demod_frames_result_t *res = p.res;
    if (t == 0) s_best = kAcqNone;
    const int phase = acquire_final_phase(p.part, p.grid, R, res->metric, s_acc, s_m, &s_phase);
    {
        unsigned long long v = kAcqNone;
        for (int b = t; b < p.grid; b += kAcqThreads) {
            const unsigned long long f = p.tail[(long long)b * R + phase];
            v = f < v ? f : v;
        }
        if (v != kAcqNone) atomicMin(&s_best, v);   // integer, LDS
    }
    // exclusive prefix of the phase's hits per tile: thread t's chunk of tiles
    const long long tiles = (p.n_windows + kAcqTile - 1) / kAcqTile;
    const long long chunk = (tiles + kAcqThreads - 1) / kAcqThreads;
    const long long lo = t * chunk < tiles ? t * chunk : tiles;
    const long long hi = lo + chunk < tiles ? lo + chunk : tiles;
    unsigned sum = 0;
#pragma unroll 4
    for (long long i = lo; i < hi; ++i) sum += p.count[i * R + phase];
    s_chunk[t] = sum;
    __syncthreads();
    unsigned run = 0;
    for (int g = 0; g < t; ++g) run += s_chunk[g];
    for (long long i = lo; i < hi; ++i) {
        p.offs[i] = run;
        run += p.count[i * R + phase];
    }
    if (t == kAcqThreads - 1) {   // the last thread's running sum is the total
        const unsigned long long n_hits = run;
        const bool tail = s_best != kAcqNone;
        res->phases = (uint32_t)R;
        res->phase = (uint32_t)phase;
        res->per_phase = (uint64_t)p.per_phase;
        res->n_hits = n_hits;
        res->n_written = n_hits < p.max_frames ? n_hits : p.max_frames;
        res->tail_window = tail ? (int64_t)(s_best >> 8) : -1;
        res->tail_errors = tail ? (uint32_t)(s_best & 0xFF) : 0u;
        res->reserved = 0;
    }
}

__global__ __launch_bounds__(kAcqThreads) void frames_emit_kernel(FramesParams p)
{
    constexpr int kWaves = kAcqThreads / 64;
    __shared__ uint8_t s_sym[kAcqTile + kAcqHalo];
    __shared__ uint8_t s_sync[DEMOD_MAX_SYNC];
    __shared__ unsigned s_wtot[kAcqPerThread][kWaves];
    const int t = threadIdx.x, wave = t / 64, lane = t % 64;
    const int R = p.phases, L = p.sync_len, phase = (int)p.res->phase;
    const int halo = (L - 1) * R, starts = kAcqTile / R;   // starts on the phase per tile
    const long long W = p.n_windows, span = frame_span(p.sync_len, p.frame_symbols, p.phases);
    if (t < DEMOD_MAX_SYNC) s_sync[t] = p.sync[t];
    const long long tiles = (W + kAcqTile - 1) / kAcqTile;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        // the same for every thread of the block: the barriers below are uniform
        const unsigned long long off = p.offs[tile];
        if (p.count[tile * R + phase] == 0 || off >= p.max_frames) continue;
        const long long base = tile * kAcqTile;
        __syncthreads();  // the previous tile's compares have read s_sym and s_wtot
        uint8_t sv[kAcqPerThread];
        acq_stage_tile(p.sym, W, base, halo, s_sym, sv);
        __syncthreads();
        unsigned long long ballot[kAcqPerThread];
        unsigned err[kAcqPerThread];
#pragma unroll
        for (int i = 0; i < kAcqPerThread; ++i) {
            const int sidx = t + kAcqThreads * i;
            const int local = phase + sidx * R;
            bool hit = false;
            err[i] = 0;
            if (sidx < starts && base + local + span < W) {
                err[i] = acq_word_errors(s_sym, s_sync, local, R, L, p.max_errors);
                hit = err[i] <= p.max_errors;
            }
            ballot[i] = __ballot(hit);
            if (lane == 0) s_wtot[i][wave] = (unsigned)__popcll(ballot[i]);
        }
        __syncthreads();
        unsigned long long rank = off;
#pragma unroll
        for (int i = 0; i < kAcqPerThread; ++i) {
            unsigned before = 0, all = 0;
#pragma unroll
            for (int v = 0; v < kWaves; ++v) {
                const unsigned n = s_wtot[i][v];
                before += v < wave ? n : 0;
                all += n;
            }
            if ((ballot[i] >> lane) & 1ull) {
                const unsigned long long idx =
                    rank + before + (unsigned)__popcll(ballot[i] & ((1ull << lane) - 1ull));
                if (idx < p.max_frames) {
                    demod_frame_hit_t h;
                    h.window = (uint64_t)(base + phase + (long long)(t + kAcqThreads * i) * R);
                    h.errors = err[i];
                    h.reserved = 0;
                    p.hits[idx] = h;
                }
            }
            rank += all;
        }
    }
}

__global__ __launch_bounds__(kAcqThreads) void frames_gather_kernel(FramesParams p)
{
    const unsigned long long nw = p.res->n_written, N = (unsigned long long)p.frame_symbols;
    const unsigned long long R = (unsigned long long)p.phases, L = (unsigned long long)p.sync_len;
    const unsigned long long step = (unsigned long long)gridDim.x * kAcqThreads;
    const unsigned long long first = (unsigned long long)blockIdx.x * kAcqThreads + threadIdx.x;
    if (p.payload) {
        for (unsigned long long e = first; e < nw * N; e += step) {
            const unsigned long long i = e / N, j = e - i * N;
            p.payload[e] = p.sym[p.hits[i].window + (L + j) * R];
        }
    }
    if (p.packed) {
        const unsigned bits = (unsigned)p.bits, mask = (1u << bits) - 1u;
        const unsigned long long B = (N * bits + 7) / 8;
        for (unsigned long long e = first; e < nw * B; e += step) {
            const unsigned long long i = e / B, b = e - i * B;
            p.packed[e] = frame_packed_byte(p.sym + p.hits[i].window + L * R, R, N, bits, mask, b);
        }
    }
}

hipError_t launch_frames(FramesParams p, hipStream_t s)
{
    p.grid = acquire_grid(p.n_windows);
    hipLaunchKernelGGL(frames_scan_kernel, dim3(p.grid), dim3(kAcqThreads), 0, s, p);
    hipLaunchKernelGGL(frames_final_kernel, dim3(1), dim3(kAcqThreads), 0, s, p);
    if (p.max_frames > 0) {
        hipLaunchKernelGGL(frames_emit_kernel, dim3(p.grid), dim3(kAcqThreads), 0, s, p);
        if (p.frame_symbols > 0 && (p.payload || p.packed)) {
            const unsigned long long row = (unsigned long long)p.frame_symbols;   // >= a packed row
            const unsigned long long blocks = (p.max_frames * row + kAcqThreads - 1) / kAcqThreads;
            hipLaunchKernelGGL(frames_gather_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)),
                               dim3(kAcqThreads), 0, s, p);
        }
    }
    return hipGetLastError();
}

}  // namespace fskd
