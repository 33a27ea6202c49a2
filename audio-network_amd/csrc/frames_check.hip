// frames_check.hip — checked frames (include/demod.h "checked frames",
// DESIGN.md §4.9 "Checked frames"): a pass over the rows a frame scan wrote
// (acquire_frames.hip, acquire_frames_segments.hip) that reads each row's length
// header, checks its CRC, marks rows that start inside an earlier valid frame
// and compacts the surviving rows and their data bytes. Groups, rows and the
// clamped count nw_g as frame_rows.h; every index below is bounded by the
// clamped count, max_len and the row width alone. Three launches whatever the
// counts are (two without d_body), no workspace:
//
//  check   one wave per row (frame_rows.h's walk), the CRC by crc_ops.h's
//          lane-split scheme over the byte table the workgroup builds in LDS,
//          the squares x^(8 2^j) computed once on the host and passed in the
//          parameter block. length, crc, status.
//  select  one workgroup per group walks its rows in chunks of kRowThreads,
//          carrying (rows OK, rows kept, max end so far) in registers. covered
//          is the exclusive prefix maximum of end over the OK rows against the
//          row's own window: a wave scan by shuffle, wave totals through LDS. A
//          kept row's rank is the rows kept before the chunk, in the waves
//          before (LDS) and in the lanes before (ballot), as frames_emit_kernel:
//          ascending by construction. covered, kept, summary. A frame's span on
//          the air is frame_shape.h's, coded with fec_depth (the check over
//          frames_fec.hip's rows).
//  body    one thread per data byte of the kept rows, coalesced along the byte
//          index (the same walk, a wave per 64 bytes); reads n_kept, kept and
//          length as select and check left them.
//
// The prefix maximum is deliberately not the serial greedy hold-off: it drops a
// superset of what greedy drops, and the two differ only when frames that pass
// their CRC overlap each other. No atomics; every output byte is a function of
// the inputs alone.
#include "crc_ops.h"
#include "frame_rows.h"

namespace fskd {

static_assert(kRowThreads == 256, "one thread builds one entry of the byte table");

template <int WIDTH>
__global__ __launch_bounds__(kRowThreads) void frames_check_kernel(FramesCheckParams p, unsigned wpg)
{
    __shared__ unsigned s_tab[256];
    const int lane = threadIdx.x % kRowLanes;
    crc_byte_table(s_tab, p.poly);
    __syncthreads();
    const RowWave rw = row_wave(p.n_groups, wpg);
    if (!rw.live) return;
    const unsigned g = rw.g;
    const unsigned nw = rows_clamped(p.res[g].n_written, p.max_frames);
    const unsigned h = (unsigned)p.len_bytes;
    for (unsigned i = rw.c; i < nw; i += wpg) {   // the same for every lane of the wave
        const size_t r = (size_t)g * p.max_frames + i;
        const uint8_t *row = p.packed + r * p.row_bytes;
        const unsigned len = row_length_load(row, h);
        unsigned crc = 0, status = DEMOD_CHECK_BAD_LENGTH;
        if (len <= p.max_len) {
            const unsigned n = h + len;                         // <= row_bytes - crc_bytes
            const unsigned reg = crc_wave<WIDTH>(row, n, lane, p.init, p.poly, p.xpow8, s_tab);
            crc = reg >> (32 - WIDTH);
            unsigned stored = 0;
            for (int b = 0; b < p.crc_bytes; ++b) stored = (stored << 8) | row[n + b];
            status = stored == crc ? DEMOD_CHECK_OK : DEMOD_CHECK_BAD_CRC;
        }
        if (lane == 0) {
            demod_frame_check_t *out = p.check + r;
            out->length = len;
            out->crc = crc;
            out->status = status;
        }
    }
}

__global__ __launch_bounds__(kRowThreads) void frames_select_kernel(FramesCheckParams p)
{
    __shared__ unsigned long long s_wmax[kRowWaves];
    __shared__ unsigned s_wkept[kRowWaves], s_wok[kRowWaves];
    const int t = threadIdx.x, wave = t / kRowLanes, lane = t % kRowLanes;
    const unsigned long long R = (unsigned long long)p.phases, L = (unsigned long long)p.sync_len;
    const unsigned bits = (unsigned)p.bits;
    for (unsigned g = blockIdx.x; g < p.n_groups; g += gridDim.x) {
        // the same for every thread of the block: the barriers below are uniform
        const unsigned nw = rows_clamped(p.res[g].n_written, p.max_frames);
        const size_t row0 = (size_t)g * p.max_frames;
        unsigned n_ok = 0, n_kept = 0;
        unsigned long long carry = 0;   // max end over the OK rows of the chunks before
        for (unsigned base = 0; base < nw; base += kRowThreads) {
            const unsigned i = base + t;
            const bool in = i < nw;
            bool ok = false;
            unsigned long long window = 0, end = 0;
            if (in && p.check[row0 + i].status == DEMOD_CHECK_OK) {
                ok = true;
                window = p.hits[row0 + i].window;
                // the frame's symbols on the air: its bytes, or coded 2 T(len) bits
                const unsigned S = checked_frame_span(p.check[row0 + i].length, (unsigned)p.len_bytes,
                                                      (unsigned)p.crc_bytes, bits, (unsigned)p.fec_depth, (unsigned)p.fec,
                                                      (unsigned)p.parity);
                end = window + (L + S) * R;
            }
            // inclusive maximum over the lanes up to this one, then over the waves before
            unsigned long long x = end;
            for (int d = 1; d < kRowLanes; d <<= 1) {
                const unsigned long long y = __shfl_up(x, d);
                if (lane >= d && y > x) x = y;
            }
            unsigned long long before = __shfl_up(x, 1);
            if (lane == 0) before = 0;
            if (lane == kRowLanes - 1) s_wmax[wave] = x;
            __syncthreads();
            unsigned long long all = carry;
            if (carry > before) before = carry;
#pragma unroll
            for (int v = 0; v < kRowWaves; ++v) {
                const unsigned long long m = s_wmax[v];
                if (v < wave && m > before) before = m;
                if (m > all) all = m;
            }
            const bool covered = ok && before > window;
            const bool keep = ok && !covered;
            const unsigned long long kb = __ballot(keep), ob = __ballot(ok);
            if (lane == 0) {
                s_wkept[wave] = (unsigned)__popcll(kb);
                s_wok[wave] = (unsigned)__popcll(ob);
            }
            __syncthreads();
            unsigned k_before = 0, k_all = 0, ok_all = 0;
#pragma unroll
            for (int v = 0; v < kRowWaves; ++v) {
                const unsigned n = s_wkept[v];
                k_before += v < wave ? n : 0;
                k_all += n;
                ok_all += s_wok[v];
            }
            if (in) p.check[row0 + i].covered = covered ? 1u : 0u;
            if (keep)
                p.kept[row0 + n_kept + k_before + (unsigned)__popcll(kb & ((1ull << lane) - 1ull))] = i;
            n_kept += k_all;
            n_ok += ok_all;
            carry = all;
        }
        if (t == 0) {
            demod_frames_check_result_t s;
            s.n_checked = nw;
            s.n_valid = n_ok;
            s.n_kept = n_kept;
            s.reserved = 0;
            p.summary[g] = s;
        }
    }
}

// wpg waves per group: wave c of group g takes bytes 64 c + lane, + 64 wpg, ..
__global__ __launch_bounds__(kRowThreads) void frames_body_kernel(FramesCheckParams p, unsigned wpg)
{
    const int lane = threadIdx.x % kRowLanes;
    const RowWave rw = row_wave(p.n_groups, wpg);
    if (!rw.live) return;
    const unsigned long long g = rw.g, c = rw.c;
    const unsigned long long nk = rows_clamped(p.summary[g].n_kept, p.max_frames);   // select's, of this call
    const unsigned long long M = p.max_len, B = p.row_bytes;
    const size_t row0 = (size_t)g * p.max_frames;
    const unsigned long long step = (unsigned long long)wpg * kRowLanes;
    for (unsigned long long e = c * kRowLanes + lane; e < nk * M; e += step) {
        const unsigned long long r = e / M, b = e - r * M;
        const unsigned i = p.kept[row0 + r];
        if (i < p.max_frames && b < p.check[row0 + i].length)
            p.body[(row0 + r) * M + b] = p.packed[(row0 + i) * B + p.len_bytes + b];
    }
}

hipError_t launch_frames_check(const FramesCheckParams &p, hipStream_t s)
{
    const unsigned S = p.n_groups, wpg = row_waves_per_group(S, p.max_frames);
    if (p.crc_bytes == 2)
        hipLaunchKernelGGL(frames_check_kernel<16>, dim3(row_blocks(S, wpg)), dim3(kRowThreads), 0, s, p, wpg);
    else
        hipLaunchKernelGGL(frames_check_kernel<32>, dim3(row_blocks(S, wpg)), dim3(kRowThreads), 0, s, p, wpg);
    hipLaunchKernelGGL(frames_select_kernel, dim3(S), dim3(kRowThreads), 0, s, p);
    if (p.body && p.max_len > 0) {   // a wave per 64 bytes of a group's bodies
        const unsigned long long want = ((unsigned long long)p.max_frames * p.max_len + kRowLanes - 1) / kRowLanes;
        const unsigned bwpg = row_waves_per_group(S, want);
        hipLaunchKernelGGL(frames_body_kernel, dim3(row_blocks(S, bwpg)), dim3(kRowThreads), 0, s, p, bwpg);
    }
    return hipGetLastError();
}

__global__ __launch_bounds__(kRowThreads) void frames_kept_rows_kernel(
    const demod_frame_hit_t *hits, const demod_frame_check_t *check, const uint32_t *kept,
    const demod_frames_check_result_t *summary, unsigned max_frames, demod_frame_hit_t *out_hits,
    uint32_t *out_len)
{
    const unsigned long long nk = rows_clamped(summary->n_kept, max_frames);
    const unsigned long long step = (unsigned long long)gridDim.x * kRowThreads;
    for (unsigned long long r = (unsigned long long)blockIdx.x * kRowThreads + threadIdx.x; r < nk; r += step) {
        const unsigned i = kept[r];
        if (i >= max_frames) continue;
        out_hits[r] = hits[i];
        out_len[r] = check[i].length;
    }
}

hipError_t launch_frames_kept_rows(const demod_frame_hit_t *hits, const demod_frame_check_t *check,
                                   const uint32_t *kept, const demod_frames_check_result_t *summary,
                                   unsigned max_frames, demod_frame_hit_t *out_hits, uint32_t *out_len,
                                   hipStream_t s)
{
    const unsigned blocks = (max_frames + kRowThreads - 1) / kRowThreads;
    hipLaunchKernelGGL(frames_kept_rows_kernel, dim3(blocks < 1024 ? blocks : 1024), dim3(kRowThreads), 0, s,
                       hits, check, kept, summary, max_frames, out_hits, out_len);
    return hipGetLastError();
}

}  // namespace fskd
