// acquire_segments.hip — the acquisition of acquire.hip over S segments of one
// batch in one call (include/demod.h "segmented acquisition", DESIGN.md §4.9
// "Segments"). Segment s is batch windows first[s] .. first[s] + count[s] - 1
// and is treated exactly as a batch of its own: its own phase metric, phase,
// sync word position and symbol-rate row. The tables are device memory, so the
// kernels clamp them (first' = min(first, Wb), count' = min(count, Wb - first'))
// and every index below is bounded by the clamped values alone.
//
// The unit of work is a segment-relative tile of kAcqTile windows, taken by ONE
// WAVE: the workload is many short segments (a 60 ms packet is ~11 windows at
// hop 256), and a wave per tile puts four segments in a workgroup where a
// workgroup per tile would idle 245 threads; a 4 M-window segment is 4096
// tiles, i.e. 4096 waves. 64 is a multiple of R (a power of two <= 64), so
// lane l's windows l + 64 i of a tile are all on phase l mod R, relative to the
// segment's start.
//
//  plan      one workgroup: clamps the tables, counts each segment's tiles (0
//            for fewer than R windows) and writes to d_work the clamped table,
//            the exclusive prefix of tiles and the call's total. A segment is
//            kept while the tiles of segments 0 .. s together fit the
//            workspace's tile budget; the others are reported as short ones.
//  scan      waves walk the call's tiles (wave-stride), find (segment, tile)
//            by binary search in the prefix, add the decided tone's power per
//            lane in window order, then across the lanes of a phase by a
//            butterfly (xor 32, 16, .. R: a fixed tree). The sync word is
//            compared from LDS (the tile's symbols and the (sync_len - 1) R
//            after it, 0xFF past the segment's end); a lane's windows ascend,
//            so its first match is its lowest, and the butterfly takes the
//            minimum. One partial and one first-match word per phase per tile
//            go to d_work by plain stores.
//  finalise  one wave per segment: its tiles' partials [tiles][R] read as one
//            array, lane l adding entries l, l + 64, .., then the butterfly;
//            segments of more than kSegWaveTiles tiles are added by the whole
//            workgroup instead (thread t entries t, t + 256, .., then thread r
//            its phase's threads in order, as acquire_final_kernel; the
//            first-match words of its phase likewise, an integer atomicMin in
//            LDS). Argmax with ties to the lowest phase, the phase's lowest
//            first-match word, every byte of result[s].
//  gather    out[s cap + j] = sym[first' + first_window + j R], j < n_written.
//
// The scan's tile body and the finaliser's phase decision are in
// acquire_seg_scan.h, shared with acquire_frames_segments.hip.
//
// Every sum's order depends on the segment's (count, R) alone: not on first[s],
// the slot s, S or the grid. No floating-point atomics. Every word of d_work a
// launch reads was stored by an earlier launch of the same call.
#include "acquire_seg_scan.h"
#include "frame_rows.h"

static_assert(fskd::kSegWaves == fskd::kRowWaves, "the gathers are launched by frame_rows.h's arithmetic");

namespace fskd {

constexpr int kSegPlanThreads = 1024;

__global__ __launch_bounds__(kSegPlanThreads) void acquire_seg_plan_kernel(AcquireSegParams p)
{
    __shared__ unsigned long long s_wave[kSegPlanThreads / kSegLanes];
    __shared__ unsigned s_total;
    const int t = threadIdx.x, wave = t / kSegLanes, lane = t % kSegLanes;
    const unsigned long long Wb = (unsigned long long)p.n_windows;
    if (t == 0) s_total = 0;
    unsigned long long carry = 0;   // tiles of the segments before this round (same in every thread)
    for (unsigned base = 0; base < p.n_segments; base += kSegPlanThreads) {
        const unsigned s = base + t;
        const bool in = s < p.n_segments;
        unsigned long long f = 0, c = 0, tiles = 0;
        if (in) {
            f = p.seg_first[s];
            f = f < Wb ? f : Wb;
            c = p.seg_count[s];
            c = c < Wb - f ? c : Wb - f;
            tiles = c >= (unsigned long long)p.phases ? (c + kAcqTile - 1) / kAcqTile : 0;
        }
        unsigned long long x = tiles;   // inclusive scan within the wave
        for (int d = 1; d < kSegLanes; d <<= 1) {
            const unsigned long long y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == kSegLanes - 1) s_wave[wave] = x;
        __syncthreads();
        unsigned long long before = 0, all = 0;
        for (int w = 0; w < kSegPlanThreads / kSegLanes; ++w) {
            const unsigned long long v = s_wave[w];
            before += w < wave ? v : 0;
            all += v;
        }
        if (in) {
            const unsigned long long incl = carry + before + x, excl = incl - tiles;
            const bool kept = tiles > 0 && incl <= p.budget;
            p.w_first[s] = f;
            p.w_count[s] = (unsigned)c;
            p.w_tile0[s] = excl < 0xFFFFFFFFull ? (unsigned)excl : 0xFFFFFFFFu;
            p.w_tiles[s] = kept ? (unsigned)tiles : 0u;
            if (kept) atomicMax(&s_total, (unsigned)incl);   // integer, LDS
        }
        carry += all;
        __syncthreads();  // s_wave is rewritten by the next round
    }
    __syncthreads();
    if (t == 0) *p.w_total = s_total;
}

__global__ __launch_bounds__(kSegThreads) void acquire_seg_scan_kernel(AcquireSegParams p)
{
    __shared__ uint8_t s_sym[kSegWaves][kAcqTile + kSegHalo];
    __shared__ uint8_t s_sync[DEMOD_MAX_SYNC];
    const int t = threadIdx.x, wave = t / kSegLanes, lane = t % kSegLanes;
    const int R = p.phases;
    if (t < DEMOD_MAX_SYNC) s_sync[t] = p.sync[t];
    const unsigned total = *p.w_total;
    for (unsigned g0 = blockIdx.x * kSegWaves; g0 < total; g0 += gridDim.x * kSegWaves) {
        const unsigned g = g0 + wave;
        const SegTile tl = seg_tile_of(p, g, total);
        const SegScan r = seg_scan_tile<false>(p, tl, s_sym[wave], s_sync, lane, 0);
        if (tl.live && lane < R) {
            p.part[(size_t)g * R + lane] = r.acc;
            p.first[(size_t)g * R + lane] = r.word;
        }
    }
}

__global__ __launch_bounds__(kSegThreads) void acquire_seg_final_kernel(AcquireSegParams p)
{
    __shared__ SegFinalLds lds;
    const int lane = threadIdx.x % kSegLanes, R = p.phases;
    const SegFinal fin = seg_final_phase(p, lds);
    if (!fin.valid) return;
    const unsigned nt = fin.nt;
    const unsigned long long cnt = fin.cnt, best = fin.best;
    const int phase = fin.phase;
    demod_acquire_result_t *res = p.res + fin.s;
    res->metric[lane] = (lane < R && nt > 0) ? fin.m : 0.0;
    if (lane == 0) {
        const bool is_short = nt == 0;   // fewer than R windows, or past the tile budget
        const bool found = !is_short && p.sync_len > 0 && best != kSegNone;
        unsigned long long fw = (unsigned long long)phase;
        if (p.sync_len > 0) fw = found ? (best >> 8) + (unsigned long long)p.sync_len * R : cnt;
        if (is_short) fw = cnt;
        const unsigned long long n_out = fw < cnt ? (cnt - fw + R - 1) / R : 0;
        res->phases = (uint32_t)R;
        res->phase = is_short ? 0u : (uint32_t)phase;
        res->per_phase = is_short ? 0u : (uint64_t)(cnt / R);
        res->sync_window = found ? (int64_t)(best >> 8) : -1;
        res->sync_errors = found ? (uint32_t)(best & 0xFF) : 0u;
        res->reserved = 0;
        res->first_window = fw;
        res->n_out = n_out;
        res->n_written = n_out < p.cap ? n_out : p.cap;
    }
}

// wps waves per segment: wave c of segment s writes j = 64 c + lane, + 64 wps, ..
__global__ __launch_bounds__(kSegThreads) void acquire_seg_gather_kernel(AcquireSegParams p, unsigned wps)
{
    const int wave = threadIdx.x / kSegLanes, lane = threadIdx.x % kSegLanes;
    const unsigned long long gw = (unsigned long long)blockIdx.x * kSegWaves + wave;
    const unsigned long long s = gw / wps, c = gw % wps;
    if (s >= p.n_segments) return;
    const unsigned long long n = p.res[s].n_written, fw = p.w_first[s] + p.res[s].first_window;
    uint8_t *row = p.out + s * p.cap;
    for (unsigned long long j = c * kSegLanes + lane; j < n; j += (unsigned long long)wps * kSegLanes)
        row[j] = p.sym[fw + j * p.phases];
}

void launch_acquire_seg_plan(const AcquireSegParams &p, hipStream_t s)
{
    hipLaunchKernelGGL(acquire_seg_plan_kernel, dim3(1), dim3(kSegPlanThreads), 0, s, p);
}

hipError_t launch_acquire_segments(const AcquireSegParams &p, hipStream_t s)
{
    const unsigned S = p.n_segments;
    launch_acquire_seg_plan(p, s);
    hipLaunchKernelGGL(acquire_seg_scan_kernel, dim3(seg_tile_grid(p.budget)), dim3(kSegThreads), 0, s, p);
    hipLaunchKernelGGL(acquire_seg_final_kernel, dim3((S + kSegWaves - 1) / kSegWaves),
                       dim3(kSegThreads), 0, s, p);
    if (p.cap > 0) {
        const unsigned wps = row_waves_per_group(S, (p.cap + kSegLanes - 1) / kSegLanes);   // frame_rows.h
        hipLaunchKernelGGL(acquire_seg_gather_kernel, dim3(row_blocks(S, wps)), dim3(kSegThreads), 0, s, p, wps);
    }
    return hipGetLastError();
}

}  // namespace fskd
