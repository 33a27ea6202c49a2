// frames_carry.hip — the receiver's device-resident carry (include/demod.h
// "receiver", DESIGN.md §4.9 "Receiver"): what turns the one-batch frame stages
// into a receiver of live streams. Per stream a run X of detector outputs
// (sym[i], P[i][K], i < fill) lives in one slot of a [S][C] ring; a push moves
// the windows still needed and the packet's new ones into the other ring
// (advance), the segmented frame scan and the check run on that ring as a batch
// of S segments, and collect turns the check's sparse per-stream outputs into
// one dense list. State and tables are device memory: every launch reads and
// clamps them itself (keep <= fill <= C, first and count into the batch, stored
// counts to max_frames, lengths to max_len), and every index below is bounded
// by the clamped values alone. No floating-point operation (the powers move as
// 32-bit words), no atomics; every output byte is a function of the inputs.
//
// advance, two launches whatever S and the counts are:
//  copy    wps waves per stream (frame_rows.h's walk, a wave per 64 elements).
//          Output position j of stream s is Y[j + d]: the
//          old ring's window keep' + j + d while that is below fill, else the
//          packet's window first' + (j + d - kept). Wave c takes elements 64 c +
//          lane, + 64 wps, .. of the slot's fill' K power words and then of its
//          fill' symbol bytes: consecutive lanes, consecutive addresses on both
//          sides (one seam per stream). Positions at or past fill' are left.
//  state   one thread per stream rewrites base, dropped, fill and keep (0: it is
//          consumed) and the scan's tables {s C, fill'}. The copy launch reads
//          the state this launch replaces, so it runs first.
//
// collect, three launches whatever S and the counts are:
//  stream  one wave per stream: the largest end over the OK rows (the check's
//          span, checked_frame_span) into hold, keep from the scan's tail
//          less R - 1 windows, cut_hits; the stream's emitted rows and their bytes into d_work, with
//          the hold the decision used.
//  prefix  one workgroup: thread t sums a contiguous chunk of streams, the chunk
//          totals go through LDS and each thread rewrites its chunk as the
//          exclusive prefix (frames_final_kernel's scheme, over S <= 65536 = 256
//          chunks of 256); the last thread's running sums are the totals.
//  write   one wave per stream walks its kept rows again, 64 at a time: a row's
//          rank is the stream's prefix, the chunks before and the popcount of
//          the ballot below the lane; its body offset the same with a wave scan
//          of the lengths. The record is stored, then the wave copies the
//          chunk's bodies one after the other, 64 consecutive bytes a step.
#include "frame_rows.h"

namespace fskd {

// Step 1 of one stream, from the state and the tables as they are stored.
struct RxMove {
    unsigned keep;             // keep' = min(keep, fill), fill clamped to C
    unsigned kept;             // fill - keep'
    unsigned long long first;  // the packet's first window, clamped into the batch
    unsigned long long drop;   // d: the oldest windows of Y that go
    unsigned fill;             // len(Y) - d <= C
};

static __device__ __forceinline__ RxMove rx_move(const RxAdvanceParams &p, unsigned s)
{
    RxMove m;
    const unsigned fill = p.state[s].fill < p.ring ? p.state[s].fill : p.ring;
    m.keep = p.state[s].keep < fill ? p.state[s].keep : fill;
    m.kept = fill - m.keep;
    const unsigned long long f = p.new_first[s];
    m.first = f < p.n_new ? f : p.n_new;
    const unsigned long long c = p.new_count[s];
    const unsigned long long cnt = c < p.n_new - m.first ? c : p.n_new - m.first;
    const unsigned long long len = m.kept + cnt;
    m.drop = len > p.ring ? len - p.ring : 0ull;
    m.fill = (unsigned)(len - m.drop);
    return m;
}

__global__ __launch_bounds__(kRowThreads) void rx_advance_copy_kernel(RxAdvanceParams p, unsigned wps)
{
    const int lane = threadIdx.x % kRowLanes;
    const RowWave rw = row_wave(p.n_streams, wps);
    if (!rw.live) return;
    const unsigned s = rw.g;
    const unsigned long long c = rw.c;
    const RxMove m = rx_move(p, s);
    const unsigned long long K = (unsigned long long)p.k;
    const unsigned long long slot = (unsigned long long)s * p.ring;
    const unsigned long long step = (unsigned long long)wps * kRowLanes, e0 = c * kRowLanes + lane;
    // the powers as 32-bit words: moved, never computed with
    const unsigned *old_mag = reinterpret_cast<const unsigned *>(p.ring_mag_in) + (slot + m.keep) * K;
    const unsigned *new_mag = reinterpret_cast<const unsigned *>(p.new_mag) + m.first * K;
    unsigned *out_mag = reinterpret_cast<unsigned *>(p.ring_mag_out) + slot * K;
    const unsigned long long seam = m.kept * K;   // words of Y that come from the old ring
    for (unsigned long long e = e0; e < m.fill * K; e += step) {
        const unsigned long long y = e + m.drop * K;
        out_mag[e] = y < seam ? old_mag[y] : new_mag[y - seam];
    }
    const uint8_t *old_sym = p.ring_sym_in + slot + m.keep;
    const uint8_t *new_sym = p.new_sym + m.first;
    uint8_t *out_sym = p.ring_sym_out + slot;
    for (unsigned long long e = e0; e < m.fill; e += step) {
        const unsigned long long y = e + m.drop;
        out_sym[e] = y < m.kept ? old_sym[y] : new_sym[y - m.kept];
    }
}

__global__ __launch_bounds__(kRowThreads) void rx_advance_state_kernel(RxAdvanceParams p)
{
    const unsigned s = blockIdx.x * kRowThreads + threadIdx.x;
    if (s >= p.n_streams) return;
    const RxMove m = rx_move(p, s);
    demod_rx_stream_state_t *st = p.state + s;
    st->base += m.keep + m.drop;
    st->dropped += m.drop;
    st->fill = m.fill;
    st->keep = 0;
    p.seg_first[s] = (unsigned long long)s * p.ring;
    p.seg_count[s] = m.fill;
}

hipError_t launch_rx_advance(const RxAdvanceParams &p, hipStream_t s)
{
    const unsigned S = p.n_streams;
    const unsigned wps = row_waves_per_group(S, ((unsigned long long)p.ring * p.k + kRowLanes - 1) / kRowLanes);
    hipLaunchKernelGGL(rx_advance_copy_kernel, dim3(row_blocks(S, wps)), dim3(kRowThreads), 0, s, p, wps);
    hipLaunchKernelGGL(rx_advance_state_kernel, dim3((S + kRowThreads - 1) / kRowThreads), dim3(kRowThreads), 0,
                       s, p);
    return hipGetLastError();
}

// ---- collect -------------------------------------------------------------------

// a row's data bytes as the record reports and the copy moves them
static __device__ __forceinline__ unsigned rx_length(const RxCollectParams &p, size_t row)
{
    const unsigned len = p.check[row].length;
    return len < p.max_len ? len : p.max_len;
}

// kept entry r of stream s: is its row emitted against `hold`? i: the row
static __device__ __forceinline__ bool rx_emitted(const RxCollectParams &p, size_t row0, unsigned r,
                                                  unsigned long long base, unsigned long long hold,
                                                  unsigned &i)
{
    i = p.kept[row0 + r];
    return i < p.max_frames && base + p.hits[row0 + i].window >= hold;
}

__global__ __launch_bounds__(kRowThreads) void rx_collect_stream_kernel(RxCollectParams p)
{
    const int wave = threadIdx.x / kRowLanes, lane = threadIdx.x % kRowLanes;
    const unsigned s = blockIdx.x * kRowWaves + wave;
    if (s >= p.n_streams) return;
    const size_t row0 = (size_t)s * p.max_frames;
    const demod_frames_result_t *res = p.res + s;
    const unsigned nw = rows_clamped(res->n_written, p.max_frames);
    const unsigned nk = rows_clamped(p.chk_sum[s].n_kept, p.max_frames);
    const unsigned long long base = p.state[s].base, hold = p.state[s].hold;
    const unsigned long long R = (unsigned long long)p.phases, L = (unsigned long long)p.sync_len;
    unsigned long long reach = hold;   // max(hold, the largest end over the OK rows)
    for (unsigned i = lane; i < nw; i += kRowLanes) {
        if (p.check[row0 + i].status != DEMOD_CHECK_OK) continue;
        const unsigned S = checked_frame_span(rx_length(p, row0 + i), (unsigned)p.len_bytes,
                                              (unsigned)p.crc_bytes, (unsigned)p.bits, (unsigned)p.fec_depth, (unsigned)p.fec,
                                              (unsigned)p.parity);
        const unsigned long long end = base + p.hits[row0 + i].window + (L + S) * R;
        if (end > reach) reach = end;
    }
    unsigned cnt = 0;
    unsigned long long bytes = 0;
    for (unsigned r = lane; r < nk; r += kRowLanes) {
        unsigned i;
        if (rx_emitted(p, row0, r, base, hold, i)) {
            ++cnt;
            bytes += rx_length(p, row0 + i);
        }
    }
    for (int d = kRowLanes / 2; d > 0; d >>= 1) {
        const unsigned long long y = __shfl_xor(reach, d);
        if (y > reach) reach = y;
        cnt += __shfl_xor(cnt, d);
        bytes += __shfl_xor(bytes, d);
    }
    if (lane != 0) return;
    p.w_hold[s] = hold;
    p.w_cnt[s] = cnt;
    p.w_bytes[s] = bytes;
    demod_rx_stream_state_t *st = p.state + s;
    const unsigned fill = st->fill;
    const long long tail = res->tail_window;
    const unsigned long long word = (L - 1) * R;   // a start at or past fill - word: its word does not fit yet
    unsigned keep = fill > word ? (unsigned)(fill - word) : 0u;
    if (tail >= 0) keep = (unsigned long long)tail < fill ? (unsigned)tail : fill;
    // R - 1 windows more: the same word's start on the neighbouring earlier phases, should the next push choose one
    const unsigned back = (unsigned)(R - 1);
    st->hold = reach;
    st->keep = keep > back ? keep - back : 0u;
    const unsigned long long n_hits = res->n_hits, n_written = res->n_written;
    st->cut_hits += n_hits > n_written ? n_hits - n_written : 0ull;
}

__global__ __launch_bounds__(kRowThreads) void rx_collect_prefix_kernel(RxCollectParams p)
{
    __shared__ unsigned s_cnt[kRowThreads];
    __shared__ unsigned long long s_bytes[kRowThreads], s_checked[kRowThreads], s_valid[kRowThreads];
    const unsigned t = threadIdx.x, S = p.n_streams;
    const unsigned chunk = (S + kRowThreads - 1) / kRowThreads;
    const unsigned lo = t * chunk < S ? t * chunk : S;
    const unsigned hi = lo + chunk < S ? lo + chunk : S;
    unsigned cnt = 0;
    unsigned long long bytes = 0, checked = 0, valid = 0;
    for (unsigned s = lo; s < hi; ++s) {
        cnt += p.w_cnt[s];
        bytes += p.w_bytes[s];
        checked += rows_clamped(p.chk_sum[s].n_checked, p.max_frames);
        valid += rows_clamped(p.chk_sum[s].n_valid, p.max_frames);
    }
    s_cnt[t] = cnt;
    s_bytes[t] = bytes;
    s_checked[t] = checked;
    s_valid[t] = valid;
    __syncthreads();
    unsigned run = 0;
    unsigned long long brun = 0;
    for (unsigned g = 0; g < t; ++g) {
        run += s_cnt[g];
        brun += s_bytes[g];
    }
    for (unsigned s = lo; s < hi; ++s) {
        const unsigned c = p.w_cnt[s];
        const unsigned long long b = p.w_bytes[s];
        p.w_cnt[s] = run;
        p.w_bytes[s] = brun;
        run += c;
        brun += b;
    }
    if (t == kRowThreads - 1) {   // the last thread's running sums are the totals
        unsigned long long nc = 0, nv = 0;
        for (unsigned g = 0; g < kRowThreads; ++g) {
            nc += s_checked[g];
            nv += s_valid[g];
        }
        demod_rx_summary_t sum;
        sum.n_frames = run;
        sum.n_bytes = brun;
        sum.n_checked = nc;
        sum.n_valid = nv;
        *p.summary = sum;
    }
}

__global__ __launch_bounds__(kRowThreads) void rx_collect_write_kernel(RxCollectParams p)
{
    const int wave = threadIdx.x / kRowLanes, lane = threadIdx.x % kRowLanes;
    const unsigned s = blockIdx.x * kRowWaves + wave;
    if (s >= p.n_streams) return;
    const size_t row0 = (size_t)s * p.max_frames;
    const unsigned nk = rows_clamped(p.chk_sum[s].n_kept, p.max_frames);
    const unsigned long long base = p.state[s].base, hold = p.w_hold[s];
    unsigned long long rank = p.w_cnt[s], off = p.w_bytes[s];
    const unsigned long long M = p.max_len;
    for (unsigned r0 = 0; r0 < nk; r0 += kRowLanes) {   // the same for every lane of the wave
        const unsigned r = r0 + lane;
        unsigned i = 0;
        const bool emit = r < nk && rx_emitted(p, row0, r, base, hold, i);
        const unsigned len = emit ? rx_length(p, row0 + i) : 0u;
        unsigned x = len;   // inclusive sum of the lengths over the lanes up to this one
        for (int d = 1; d < kRowLanes; d <<= 1) {
            const unsigned y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        const unsigned long long ballot = __ballot(emit);
        const unsigned long long at = off + (x - len);
        if (emit) {
            demod_rx_frame_t f;
            f.stream = s;
            f.length = len;
            f.window = base + p.hits[row0 + i].window;
            f.body = at;
            f.errors = p.hits[row0 + i].errors;
            f.reserved = 0;
            p.frames[rank + (unsigned)__popcll(ballot & ((1ull << lane) - 1ull))] = f;
        }
        // the chunk's bodies one after the other: body row r of the check is kept entry r's
        for (unsigned long long m = ballot; m != 0; m &= m - 1) {
            const int src = __ffsll((long long)m) - 1;
            const unsigned long long dst = __shfl(at, src);
            const unsigned n = __shfl(len, src);
            const uint8_t *from = p.body + (row0 + r0 + (unsigned)src) * M;
            for (unsigned b = lane; b < n; b += kRowLanes) p.bodies[dst + b] = from[b];
        }
        rank += (unsigned)__popcll(ballot);
        off += __shfl(x, kRowLanes - 1);
    }
}

hipError_t launch_rx_collect(const RxCollectParams &p, hipStream_t s)
{
    const unsigned blocks = (p.n_streams + kRowWaves - 1) / kRowWaves;
    hipLaunchKernelGGL(rx_collect_stream_kernel, dim3(blocks), dim3(kRowThreads), 0, s, p);
    hipLaunchKernelGGL(rx_collect_prefix_kernel, dim3(1), dim3(kRowThreads), 0, s, p);
    hipLaunchKernelGGL(rx_collect_write_kernel, dim3(blocks), dim3(kRowThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace fskd
