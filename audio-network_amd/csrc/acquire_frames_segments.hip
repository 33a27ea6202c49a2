// acquire_frames_segments.hip — the frame scan of acquire_frames.hip over S
// segments of one batch in one call (include/demod.h "segmented frame scan",
// DESIGN.md §4.9 "Frame segments"). Segment s is batch windows first[s] ..
// first[s] + count[s] - 1 and is scanned exactly as a batch of its own: its own
// phase decision, then EVERY sync-word hit on that phase in ascending window
// order, each with a fixed-length payload. The tables are device memory and are
// clamped by the plan launch; every index below is bounded by the clamped
// values alone. Five launches whatever S and the hit count are (four without
// payload outputs, three when max_frames == 0):
//
//  plan      acquire_segments.hip's, as it is: the clamped table, the exclusive
//            prefix of tiles and the call's total in d_work's header.
//  scan      acquire_seg_scan.h's tile body, so the phase sums are bit-identical
//            to demod_acquire_segments_async's. The phase is not known yet, so
//            a match is kept for its own phase: a complete hit (word and
//            payload inside the segment) is counted in a lane register; a
//            lane's windows ascend, so its first incomplete hit is its lowest
//            and ends its compares. Counts and tail words go through the same
//            xor butterfly as the sums (integer add, integer min); part, count
//            and tail [tile][R] are written by plain stores.
//  finalise  one wave per segment, or the workgroup for more than 64 tiles
//            (seg_final_phase: sums, argmax, the phase's lowest tail word);
//            then the exclusive prefix of the phase's counts over the segment's
//            own tiles into offs[tile] (a wave scan, or chunks per thread and
//            chunk totals through LDS as frames_final_kernel); every byte of
//            result[s].
//  emit      waves walk the call's tiles again; a tile is touched only when it
//            holds hits of its segment's phase below max_frames (wave-uniform;
//            the loop's barriers do not depend on it). The tile is staged in
//            the wave's slab, only the 1024 / R starts on the phase compared
//            (start l + 64 i in round i); a hit's rank is offs[tile], the
//            rounds before and the popcount of the ballot below the lane:
//            ascending w by construction. hits[s max_frames + rank] is stored
//            when rank < max_frames.
//  gather    a bounded number of waves per segment, each looping over its
//            segment's n_written N symbols / n_written B packed bytes (read
//            from device memory), so a batch without hits costs one load per
//            segment. Byte assembly as frames_gather_kernel (frame_packed_byte).
//
// Every output byte of a segment depends on its contents and (count', R) alone.
// No floating-point atomics, no atomics on d_work, none that decide a position;
// every word of d_work a launch reads was stored by an earlier launch of the
// same call.
#include "acquire_seg_scan.h"
#include "frame_rows.h"

static_assert(fskd::kSegWaves == fskd::kRowWaves, "the gathers are launched by frame_rows.h's arithmetic");

namespace fskd {

__global__ __launch_bounds__(kSegThreads) void frames_seg_scan_kernel(FrameSegParams q)
{
    __shared__ uint8_t s_sym[kSegWaves][kAcqTile + kSegHalo];
    __shared__ uint8_t s_sync[DEMOD_MAX_SYNC];
    const AcquireSegParams &p = q.seg;
    const int t = threadIdx.x, wave = t / kSegLanes, lane = t % kSegLanes;
    const int R = p.phases;
    const long long span = frame_span(q.seg.sync_len, q.frame_symbols, q.seg.phases);
    if (t < DEMOD_MAX_SYNC) s_sync[t] = p.sync[t];
    const unsigned total = *p.w_total;
    for (unsigned g0 = blockIdx.x * kSegWaves; g0 < total; g0 += gridDim.x * kSegWaves) {
        const unsigned g = g0 + wave;
        const SegTile tl = seg_tile_of(p, g, total);
        const SegScan r = seg_scan_tile<true>(p, tl, s_sym[wave], s_sync, lane, span);
        if (tl.live && lane < R) {
            p.part[(size_t)g * R + lane] = r.acc;
            p.first[(size_t)g * R + lane] = r.word;
            q.count[(size_t)g * R + lane] = r.count;
        }
    }
}

__global__ __launch_bounds__(kSegThreads) void frames_seg_final_kernel(FrameSegParams q)
{
    __shared__ SegFinalLds lds;
    __shared__ unsigned s_chunk[kSegThreads];
    __shared__ unsigned s_hits[kSegWaves];
    const AcquireSegParams &p = q.seg;
    const int t = threadIdx.x, wave = t / kSegLanes, lane = t % kSegLanes, R = p.phases;
    const SegFinal fin = seg_final_phase(p, lds);
    // exclusive prefix of the phase's complete hits over the segment's own tiles
    unsigned n_hits = 0;
    if (fin.nt <= kSegWaveTiles) {   // (a short segment: no tile, nothing read or stored)
        const bool in = (unsigned)lane < fin.nt;
        const unsigned c = in ? q.count[((size_t)fin.t0 + lane) * R + fin.phase] : 0u;
        unsigned x = c;
        for (int d = 1; d < kSegLanes; d <<= 1) {
            const unsigned y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (in) q.offs[fin.t0 + lane] = x - c;
        n_hits = __shfl(x, kSegLanes - 1);
    }
    // long segments: the whole workgroup, one after the other (uniform branches);
    // thread t a contiguous chunk of tiles, the chunk totals through LDS
    for (int w = 0; w < kSegWaves; ++w) {
        const unsigned ntw = lds.nt[w];
        if (ntw <= kSegWaveTiles) continue;
        const unsigned *cnt = q.count + (size_t)lds.t0[w] * R + lds.phase[w];
        unsigned *offs = q.offs + lds.t0[w];
        const unsigned chunk = (ntw + kSegThreads - 1) / kSegThreads;
        const unsigned lo = (unsigned)t * chunk < ntw ? (unsigned)t * chunk : ntw;
        const unsigned hi = lo + chunk < ntw ? lo + chunk : ntw;
        unsigned sum = 0;
#pragma unroll 4
        for (unsigned i = lo; i < hi; ++i) sum += cnt[(size_t)i * R];
        s_chunk[t] = sum;
        __syncthreads();
        unsigned run = 0;
        for (int g = 0; g < t; ++g) run += s_chunk[g];
        for (unsigned i = lo; i < hi; ++i) {
            offs[i] = run;
            run += cnt[(size_t)i * R];
        }
        if (t == kSegThreads - 1) s_hits[w] = run;   // the last thread's running sum is the total
        __syncthreads();  // s_chunk is rewritten by the next long segment
    }
    if (fin.nt > kSegWaveTiles) n_hits = s_hits[wave];
    if (!fin.valid) return;
    demod_frames_result_t *res = q.res + fin.s;
    res->metric[lane] = (lane < R && fin.nt > 0) ? fin.m : 0.0;
    if (lane == 0) {
        const bool is_short = fin.nt == 0;   // fewer than R windows, or past the tile budget
        const bool tail = !is_short && fin.best != kSegNone;
        const unsigned long long n = is_short ? 0ull : (unsigned long long)n_hits;
        res->phases = (uint32_t)R;
        res->phase = is_short ? 0u : (uint32_t)fin.phase;
        res->per_phase = is_short ? 0u : (uint64_t)(fin.cnt / R);
        res->n_hits = n;
        res->n_written = n < q.max_frames ? n : q.max_frames;
        res->tail_window = tail ? (int64_t)(fin.best >> 8) : -1;
        res->tail_errors = tail ? (uint32_t)(fin.best & 0xFF) : 0u;
        res->reserved = 0;
    }
}

__global__ __launch_bounds__(kSegThreads) void frames_seg_emit_kernel(FrameSegParams q)
{
    __shared__ uint8_t s_sym[kSegWaves][kAcqTile + kSegHalo];
    __shared__ uint8_t s_sync[DEMOD_MAX_SYNC];
    const AcquireSegParams &p = q.seg;
    const int t = threadIdx.x, wave = t / kSegLanes, lane = t % kSegLanes;
    const int R = p.phases, L = p.sync_len;
    const int halo = (L - 1) * R, starts = kAcqTile / R;   // starts on the phase per tile
    const int rounds = (starts + kSegLanes - 1) / kSegLanes;
    const long long span = frame_span(q.seg.sync_len, q.frame_symbols, q.seg.phases);
    if (t < DEMOD_MAX_SYNC) s_sync[t] = p.sync[t];
    const unsigned total = *p.w_total;
    for (unsigned g0 = blockIdx.x * kSegWaves; g0 < total; g0 += gridDim.x * kSegWaves) {
        const unsigned g = g0 + wave;
        const SegTile tl = seg_tile_of(p, g, total);
        // the same for every lane of the wave; the barriers below do not depend on it
        bool go = false;
        int phase = 0;
        unsigned long long rank = 0;
        if (tl.live) {
            phase = (int)q.res[tl.s].phase;
            rank = q.offs[g];
            go = q.count[(size_t)g * R + phase] > 0 && rank < q.max_frames;
        }
        __syncthreads();  // the previous tile's compares have read the slab
        if (go) {
            uint8_t sv[kSegPerLane];
            seg_stage_tile(p, tl, halo, s_sym[wave], lane, true, sv);
        }
        __syncthreads();
        if (!go) continue;
        demod_frame_hit_t *row = q.hits + (size_t)tl.s * q.max_frames;
        for (int i = 0; i < rounds; ++i) {
            const int sidx = lane + kSegLanes * i;
            const int local = phase + sidx * R;
            const long long w = tl.base + local;
            bool hit = false;
            unsigned err = 0;
            if (sidx < starts && w + span < tl.cnt) {
                err = acq_word_errors(s_sym[wave], s_sync, local, R, L, p.max_errors);
                hit = err <= p.max_errors;
            }
            const unsigned long long ballot = __ballot(hit);
            if (hit) {
                const unsigned long long idx = rank + (unsigned)__popcll(ballot & ((1ull << lane) - 1ull));
                if (idx < q.max_frames) {
                    demod_frame_hit_t h;
                    h.window = (uint64_t)w;
                    h.errors = err;
                    h.reserved = 0;
                    row[idx] = h;
                }
            }
            rank += (unsigned)__popcll(ballot);
        }
    }
}

// wps waves per segment: wave c of segment s takes elements 64 c + lane, + 64 wps, ..
__global__ __launch_bounds__(kSegThreads) void frames_seg_gather_kernel(FrameSegParams q, unsigned wps)
{
    const AcquireSegParams &p = q.seg;
    const int wave = threadIdx.x / kSegLanes, lane = threadIdx.x % kSegLanes;
    const unsigned long long gw = (unsigned long long)blockIdx.x * kSegWaves + wave;
    const unsigned long long s = gw / wps, c = gw % wps;
    if (s >= p.n_segments) return;
    const unsigned long long nw = q.res[s].n_written;
    if (nw == 0) return;
    const unsigned long long N = (unsigned long long)q.frame_symbols;
    const unsigned long long R = (unsigned long long)p.phases, L = (unsigned long long)p.sync_len;
    const uint8_t *sym = p.sym + p.w_first[s];
    const demod_frame_hit_t *hits = q.hits + s * q.max_frames;
    const unsigned long long step = (unsigned long long)wps * kSegLanes;
    const unsigned long long first = c * kSegLanes + lane;
    if (q.payload) {
        uint8_t *dst = q.payload + s * q.max_frames * N;
        for (unsigned long long e = first; e < nw * N; e += step) {
            const unsigned long long i = e / N, j = e - i * N;
            dst[e] = sym[hits[i].window + (L + j) * R];
        }
    }
    if (q.packed) {
        const unsigned bits = (unsigned)q.bits, mask = (1u << bits) - 1u;
        const unsigned long long B = (N * bits + 7) / 8;
        uint8_t *dst = q.packed + s * q.max_frames * B;
        for (unsigned long long e = first; e < nw * B; e += step) {
            const unsigned long long i = e / B, b = e - i * B;
            dst[e] = frame_packed_byte(sym + hits[i].window + L * R, R, N, bits, mask, b);
        }
    }
}

hipError_t launch_frames_segments(const FrameSegParams &q, hipStream_t s)
{
    const unsigned S = q.seg.n_segments;
    const unsigned grid = seg_tile_grid(q.seg.budget);
    launch_acquire_seg_plan(q.seg, s);
    hipLaunchKernelGGL(frames_seg_scan_kernel, dim3(grid), dim3(kSegThreads), 0, s, q);
    hipLaunchKernelGGL(frames_seg_final_kernel, dim3((S + kSegWaves - 1) / kSegWaves), dim3(kSegThreads),
                       0, s, q);
    if (q.max_frames > 0) {
        hipLaunchKernelGGL(frames_seg_emit_kernel, dim3(grid), dim3(kSegThreads), 0, s, q);
        if (q.frame_symbols > 0 && (q.payload || q.packed)) {
            const unsigned long long row = q.max_frames * (unsigned long long)q.frame_symbols;   // >= a packed row
            const unsigned wps = row_waves_per_group(S, (row + kSegLanes - 1) / kSegLanes);   // frame_rows.h
            hipLaunchKernelGGL(frames_seg_gather_kernel, dim3(row_blocks(S, wps)), dim3(kSegThreads), 0, s, q, wps);
        }
    }
    return hipGetLastError();
}

}  // namespace fskd
