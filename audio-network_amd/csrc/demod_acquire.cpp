// demod_acquire.cpp — the C ABI of acquisition and the frame scan on the
// detector's outputs (include/demod.h), each whole and segmented. Each has a
// workspace-size function, an *_async call on device memory and the caller's
// stream, and a synchronous wrapper that stages host or device samples, runs the
// detector (enqueue_batch, demod_api.cpp) and the scan on the handle's stream
// and copies the results. The stages over a scan's rows are demod_frames.cpp's,
// the receiver's demod_rx.cpp's.
#include <algorithm>
#include <cstring>

#include "demod_host.h"

using namespace fskd;

// The sync word and the scan fields that AcquireParams, AcquireSegParams and
// FramesParams share (FrameSegParams: its .seg).
template <class P>
static void fill_scan_fields(P &p, const demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                             size_t n_windows, uint32_t R, const uint8_t *sync, size_t sync_len,
                             uint32_t max_errors)
{
    for (size_t i = 0; i < sync_len; ++i) p.sync[i] = sync[i];
    p.sym = d_symbols;
    p.mag = d_mags;
    p.n_windows = (long long)n_windows;
    p.phases = (int)R;
    p.k = (int)st->cfg.k;
    p.sync_len = (int)sync_len;
    p.max_errors = max_errors;
}

// What the segmented async calls ask of the segment count and the device tables.
static bool seg_call_ok(size_t n_segments, const uint64_t *d_first, const uint32_t *d_count)
{
    return n_segments != 0 && n_segments <= DEMOD_MAX_SEGMENTS && aligned8(d_first) && aligned4(d_count);
}

// The synchronous segmented calls hold the tables in host memory: false for
// what the kernels would clamp, or for more rows than the return value holds
// (row_cap each, or every row of the segment). longest: the largest count;
// cover: the windows whose workspace holds every tile.
static bool check_segment_tables(const uint64_t *first, const uint32_t *count, size_t n_segments,
                                 size_t n_windows, uint32_t R, size_t row_cap, size_t *longest,
                                 size_t *cover)
{
    unsigned long long tiles = 0, rows = 0;
    *longest = 0;
    for (size_t s = 0; s < n_segments; ++s) {
        if (count[s] < R || first[s] > n_windows || count[s] > n_windows - first[s]) return false;
        *longest = std::max<size_t>(*longest, count[s]);
        tiles += (count[s] + (size_t)kAcqTile - 1) / kAcqTile;
        rows += std::min<unsigned long long>(row_cap, count[s] / R + 1);
    }
    if (rows > 0x7FFFFFFF) return false;   // the return value is their sum at most
    // a workspace for every tile: ceil(cover / T) + S of them. Disjoint segments
    // fit cover = n_windows; overlapping ones may hold more tiles than the batch
    *cover = std::max<unsigned long long>(n_windows,
                                          tiles > n_segments ? (tiles - n_segments) * kAcqTile : 0);
    return *cover <= 0x7FFFFFFF;
}

static int upload_segment_tables(demod_t *st, const uint64_t *first, const uint32_t *count,
                                 size_t n_segments)
{
    HIP_TRY(hipMemcpyAsync(st->d_seg_first.p, first, n_segments * sizeof(uint64_t),
                           hipMemcpyHostToDevice, st->stream));
    HIP_TRY(hipMemcpyAsync(st->d_seg_count.p, count, n_segments * sizeof(uint32_t),
                           hipMemcpyHostToDevice, st->stream));
    return DEMOD_OK;
}

extern "C" {

// ---- acquisition (acquire.hip) -------------------------------------------

size_t demod_acquire_workspace_size(const demod_cfg_t *cfg)
{
    if (validate_cfg(cfg) != DEMOD_OK) return 0;
    // [kAcqMaxBlocks][R] doubles, then as many 64-bit first-match words
    return (size_t)2 * kAcqMaxBlocks * acquire_phases(*cfg) * sizeof(double);
}

int demod_acquire_async(demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                        size_t n_windows, const uint8_t *sync, size_t sync_len,
                        uint32_t max_errors, uint8_t *d_out, size_t cap,
                        demod_acquire_result_t *d_result, void *d_work, void *stream)
{
    if (!st || !d_symbols || !d_mags || !d_result || !d_work) return DEMOD_BAD_ARG;
    const uint32_t R = acquire_args(st->cfg, n_windows, sync, sync_len, max_errors, true);
    if (R == 0) return DEMOD_BAD_ARG;
    if ((cap && !d_out) || !aligned8(d_result, d_work)) return DEMOD_BAD_ARG;
    AcquireParams p;
    std::memset(&p, 0, sizeof(p));
    fill_scan_fields(p, st, d_symbols, d_mags, n_windows, R, sync, sync_len, max_errors);
    p.per_phase = (long long)(n_windows / R);
    p.cap = cap;
    p.out = d_out;
    p.res = d_result;
    p.part = static_cast<double *>(d_work);
    p.first = reinterpret_cast<unsigned long long *>(p.part + (size_t)kAcqMaxBlocks * R);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_acquire(p, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_acquire(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                  size_t sync_len, uint32_t max_errors, uint8_t *out, size_t cap,
                  demod_acquire_result_t *result)
{
    if (!st || !pcm || !result || (cap && !out) || ((uintptr_t)pcm & 15) != 0) return DEMOD_BAD_ARG;
    const uint32_t R = acquire_args(st->cfg, n_windows, sync, sync_len, max_errors, true);
    if (R == 0) return DEMOD_BAD_ARG;   // before the detector runs
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(st->d_acq_work.reserve(demod_acquire_workspace_size(&st->cfg)));  // bytes
    HIP_TRY(st->d_acq_res.reserve(1));
    const size_t dcap = hit_cap(cap, n_windows, R);
    HIP_TRY(st->d_acq_out.reserve(dcap, dcap / 4 + 16));
    int rc;
    if ((rc = stage_and_detect(st, pcm, n_windows)) != DEMOD_OK) return rc;
    rc = demod_acquire_async(st, st->d_sym.p, st->d_mag.p, n_windows, sync, sync_len, max_errors,
                             dcap ? st->d_acq_out.p : nullptr, dcap, st->d_acq_res.p,
                             st->d_acq_work.p, st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(result, st->d_acq_res.p, sizeof(*result), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    if (result->n_written)
        HIP_TRY(hipMemcpy(out, st->d_acq_out.p, result->n_written, hipMemcpyDeviceToHost));
    return (int)result->n_written;
}

// ---- segmented acquisition (acquire_segments.hip) --------------------------

size_t demod_acquire_segments_workspace_size(const demod_cfg_t *cfg, size_t max_segments,
                                             size_t max_windows)
{
    if (validate_cfg(cfg) != DEMOD_OK) return 0;
    const uint32_t R = acquire_phases(*cfg);
    if (R == 0 || max_segments == 0 || max_segments > DEMOD_MAX_SEGMENTS || max_windows > 0x7FFFFFFF)
        return 0;
    const size_t tiles = (max_windows + kAcqTile - 1) / kAcqTile + max_segments;
    return acquire_seg_header_bytes(max_segments) + tiles * acquire_seg_tile_bytes(R);
}

int demod_acquire_segments_async(demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                                 size_t n_windows, const uint64_t *d_first,
                                 const uint32_t *d_count, size_t n_segments, const uint8_t *sync,
                                 size_t sync_len, uint32_t max_errors, uint8_t *d_out, size_t cap,
                                 demod_acquire_result_t *d_results, void *d_work,
                                 size_t work_bytes, void *stream)
{
    if (!st || !d_symbols || !d_mags || !d_results || !d_work || !d_first || !d_count) return DEMOD_BAD_ARG;
    const uint32_t R = acquire_args(st->cfg, n_windows, sync, sync_len, max_errors, false);
    if (R == 0 || !seg_call_ok(n_segments, d_first, d_count)) return DEMOD_BAD_ARG;
    if ((cap && !d_out) || !aligned8(d_results, d_work)) return DEMOD_BAD_ARG;
    const size_t need = demod_acquire_segments_workspace_size(&st->cfg, n_segments, n_windows);
    if (need == 0 || work_bytes < need) return DEMOD_BAD_ARG;
    const size_t budget = (work_bytes - acquire_seg_header_bytes(n_segments)) / acquire_seg_tile_bytes(R);
    AcquireSegParams p;
    std::memset(&p, 0, sizeof(p));
    fill_scan_fields(p, st, d_symbols, d_mags, n_windows, R, sync, sync_len, max_errors);
    p.seg_first = reinterpret_cast<const unsigned long long *>(d_first);
    p.seg_count = d_count;
    p.n_segments = (unsigned)n_segments;
    p.budget = (unsigned)std::min<size_t>(budget, 0xFFFFFFFFu);
    p.cap = cap;
    p.out = d_out;
    p.res = d_results;
    carve_seg_header(p, d_work, n_segments, p.budget, R);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_acquire_segments(p, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_acquire_segments(demod_t *st, const int16_t *pcm, size_t n_windows,
                           const uint64_t *first, const uint32_t *count, size_t n_segments,
                           const uint8_t *sync, size_t sync_len, uint32_t max_errors,
                           uint8_t *out, size_t cap, demod_acquire_result_t *results)
{
    if (!st || !pcm || !results || !first || !count || (cap && !out) || ((uintptr_t)pcm & 15) != 0)
        return DEMOD_BAD_ARG;
    const uint32_t R = acquire_args(st->cfg, n_windows, sync, sync_len, max_errors, true);
    if (R == 0 || n_segments == 0 || n_segments > DEMOD_MAX_SEGMENTS) return DEMOD_BAD_ARG;
    size_t longest, cover;
    if (!check_segment_tables(first, count, n_segments, n_windows, R, cap, &longest, &cover))
        return DEMOD_BAD_ARG;
    const size_t work = demod_acquire_segments_workspace_size(&st->cfg, n_segments, cover);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(st->d_seg_work.reserve(work));  // bytes
    HIP_TRY(st->d_seg_first.reserve(n_segments));
    HIP_TRY(st->d_seg_count.reserve(n_segments));
    HIP_TRY(st->d_seg_res.reserve(n_segments));
    const size_t dcap = hit_cap(cap, longest, R);
    HIP_TRY(st->d_seg_out.reserve(dcap * n_segments, 16));
    HIP_TRY(st->h_seg_out.reserve(dcap * n_segments));
    int rc;
    if ((rc = upload_segment_tables(st, first, count, n_segments)) != DEMOD_OK) return rc;
    if ((rc = stage_and_detect(st, pcm, n_windows)) != DEMOD_OK) return rc;
    rc = demod_acquire_segments_async(st, st->d_sym.p, st->d_mag.p, n_windows, st->d_seg_first.p,
                                      st->d_seg_count.p, n_segments, sync, sync_len, max_errors,
                                      dcap ? st->d_seg_out.p : nullptr, dcap, st->d_seg_res.p,
                                      st->d_seg_work.p, work, st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(results, st->d_seg_res.p, n_segments * sizeof(*results),
                           hipMemcpyDeviceToHost, st->stream));
    // the rows through pinned staging in the same pass, then each row's written
    // bytes to the caller's [S][cap]
    if (dcap)
        HIP_TRY(hipMemcpyAsync(st->h_seg_out.p, st->d_seg_out.p, dcap * n_segments,
                               hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    unsigned long long total = 0;
    for (size_t s = 0; s < n_segments; ++s) {
        const size_t nw = (size_t)results[s].n_written;
        if (nw) std::memcpy(out + s * cap, st->h_seg_out.p + s * dcap, nw);
        total += nw;
    }
    return (int)total;
}

// ---- frame scan (acquire_frames.hip) ---------------------------------------

size_t demod_frames_workspace_size(const demod_cfg_t *cfg, size_t max_windows)
{
    if (validate_cfg(cfg) != DEMOD_OK) return 0;
    const uint32_t R = acquire_phases(*cfg);
    if (R == 0 || max_windows > 0x7FFFFFFF) return 0;
    return frames_work_bytes((max_windows + kAcqTile - 1) / kAcqTile, R);
}

int demod_frames_async(demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                       size_t n_windows, const uint8_t *sync, size_t sync_len,
                       uint32_t max_errors, size_t frame_symbols, demod_frame_hit_t *d_hits,
                       uint8_t *d_payload, uint8_t *d_packed, size_t max_frames,
                       demod_frames_result_t *d_result, void *d_work, size_t work_bytes,
                       void *stream)
{
    if (!st || !d_symbols || !d_mags || !d_result || !d_work) return DEMOD_BAD_ARG;
    const uint32_t R = frames_args(st->cfg, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames, true);
    if (R == 0 || (max_frames && !d_hits) || !aligned8(d_hits, d_result, d_work)) return DEMOD_BAD_ARG;
    const size_t need = demod_frames_workspace_size(&st->cfg, n_windows);
    if (need == 0 || work_bytes < need) return DEMOD_BAD_ARG;
    const size_t tiles = (n_windows + kAcqTile - 1) / kAcqTile;
    FramesParams p;
    std::memset(&p, 0, sizeof(p));
    fill_scan_fields(p, st, d_symbols, d_mags, n_windows, R, sync, sync_len, max_errors);
    p.per_phase = (long long)(n_windows / R);
    p.frame_symbols = (long long)frame_symbols;
    p.bits = demod_bits_per_symbol(st->cfg.k);
    p.max_frames = max_frames;
    p.hits = d_hits;
    p.payload = d_payload;
    p.packed = d_packed;
    p.res = d_result;
    p.part = static_cast<double *>(d_work);
    p.tail = reinterpret_cast<unsigned long long *>(p.part + (size_t)kAcqMaxBlocks * R);
    p.offs = reinterpret_cast<unsigned *>(p.tail + (size_t)kAcqMaxBlocks * R);
    p.count = p.offs + (tiles + 1) / 2 * 2;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_frames(p, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_frames(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                 size_t sync_len, uint32_t max_errors, size_t frame_symbols,
                 demod_frame_hit_t *hits, uint8_t *payload, uint8_t *packed, size_t max_frames,
                 demod_frames_result_t *result)
{
    if (!st || !pcm || !result || (max_frames && !hits) || ((uintptr_t)pcm & 15) != 0) return DEMOD_BAD_ARG;
    const uint32_t R = frames_args(st->cfg, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames, true);
    if (R == 0) return DEMOD_BAD_ARG;   // before the detector runs
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    const size_t N = frame_symbols, B = packed_row_bytes(N, demod_bits_per_symbol(st->cfg.k));
    const size_t work = demod_frames_workspace_size(&st->cfg, n_windows);
    HIP_TRY(st->d_frm_work.reserve(work));  // bytes
    HIP_TRY(st->d_frm_res.reserve(1));
    const size_t dcap = hit_cap(max_frames, n_windows, R);
    const bool want_payload = payload && N && dcap, want_packed = packed && N && dcap;
    HIP_TRY(st->d_frm_hits.reserve(dcap));
    if (want_payload) HIP_TRY(st->d_frm_payload.reserve(dcap * N));
    if (want_packed) HIP_TRY(st->d_frm_packed.reserve(dcap * B));
    int rc;
    if ((rc = stage_and_detect(st, pcm, n_windows)) != DEMOD_OK) return rc;
    rc = demod_frames_async(st, st->d_sym.p, st->d_mag.p, n_windows, sync, sync_len, max_errors, N,
                            dcap ? st->d_frm_hits.p : nullptr,
                            want_payload ? st->d_frm_payload.p : nullptr,
                            want_packed ? st->d_frm_packed.p : nullptr, dcap, st->d_frm_res.p,
                            st->d_frm_work.p, work, st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(result, st->d_frm_res.p, sizeof(*result), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    // the device list was cut at dcap >= every possible n_hits or at max_frames
    const size_t nw = (size_t)result->n_written;
    if (nw) {
        HIP_TRY(hipMemcpy(hits, st->d_frm_hits.p, nw * sizeof(*hits), hipMemcpyDeviceToHost));
        if (want_payload) HIP_TRY(hipMemcpy(payload, st->d_frm_payload.p, nw * N, hipMemcpyDeviceToHost));
        if (want_packed) HIP_TRY(hipMemcpy(packed, st->d_frm_packed.p, nw * B, hipMemcpyDeviceToHost));
    }
    return (int)nw;
}

// ---- segmented frame scan (acquire_frames_segments.hip) ---------------------

size_t demod_frames_segments_workspace_size(const demod_cfg_t *cfg, size_t max_segments,
                                            size_t max_windows)
{
    if (validate_cfg(cfg) != DEMOD_OK) return 0;
    const uint32_t R = acquire_phases(*cfg);
    if (R == 0 || max_segments == 0 || max_segments > DEMOD_MAX_SEGMENTS || max_windows > 0x7FFFFFFF)
        return 0;
    const size_t tiles = (max_windows + kAcqTile - 1) / kAcqTile + max_segments;
    return acquire_seg_header_bytes(max_segments) + frames_seg_tiles_bytes(tiles, R);
}

int demod_frames_segments_async(demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                                size_t n_windows, const uint64_t *d_first, const uint32_t *d_count,
                                size_t n_segments, const uint8_t *sync, size_t sync_len,
                                uint32_t max_errors, size_t frame_symbols, demod_frame_hit_t *d_hits,
                                uint8_t *d_payload, uint8_t *d_packed, size_t max_frames,
                                demod_frames_result_t *d_results, void *d_work, size_t work_bytes,
                                void *stream)
{
    if (!st || !d_symbols || !d_mags || !d_results || !d_work || !d_first || !d_count) return DEMOD_BAD_ARG;
    const uint32_t R = frames_args(st->cfg, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames, false);
    if (R == 0 || !seg_call_ok(n_segments, d_first, d_count)) return DEMOD_BAD_ARG;
    const size_t need = demod_frames_segments_workspace_size(&st->cfg, n_segments, n_windows);
    if (need == 0 || work_bytes < need) return DEMOD_BAD_ARG;
    const size_t budget = std::min<size_t>(
        frames_seg_budget(work_bytes - acquire_seg_header_bytes(n_segments), R), 0xFFFFFFFFu);
    if (!group_rows_ok(n_segments, max_frames, true)) return DEMOD_BAD_ARG;
    if ((max_frames && !d_hits) || !aligned8(d_hits, d_results, d_work)) return DEMOD_BAD_ARG;
    FrameSegParams q;
    std::memset(&q, 0, sizeof(q));
    AcquireSegParams &p = q.seg;
    fill_scan_fields(p, st, d_symbols, d_mags, n_windows, R, sync, sync_len, max_errors);
    p.seg_first = reinterpret_cast<const unsigned long long *>(d_first);
    p.seg_count = d_count;
    p.n_segments = (unsigned)n_segments;
    p.budget = (unsigned)budget;
    // the header, part and tail (= seg.first) [B][R], then count [B][R] and offs [B]
    carve_seg_header(p, d_work, n_segments, budget, R);
    q.count = reinterpret_cast<unsigned *>(p.first + budget * R);
    q.offs = q.count + (budget * R + 1) / 2 * 2;
    q.frame_symbols = (long long)frame_symbols;
    q.bits = demod_bits_per_symbol(st->cfg.k);
    q.max_frames = max_frames;
    q.hits = d_hits;
    q.payload = d_payload;
    q.packed = d_packed;
    q.res = d_results;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_frames_segments(q, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_frames_segments(demod_t *st, const int16_t *pcm, size_t n_windows, const uint64_t *first,
                          const uint32_t *count, size_t n_segments, const uint8_t *sync,
                          size_t sync_len, uint32_t max_errors, size_t frame_symbols,
                          demod_frame_hit_t *hits, uint8_t *payload, uint8_t *packed,
                          size_t max_frames, demod_frames_result_t *results)
{
    if (!st || !pcm || !results || !first || !count || (max_frames && !hits) || ((uintptr_t)pcm & 15) != 0)
        return DEMOD_BAD_ARG;
    const uint32_t R = frames_args(st->cfg, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames, true);
    if (R == 0 || n_segments == 0 || n_segments > DEMOD_MAX_SEGMENTS) return DEMOD_BAD_ARG;
    size_t longest, cover;
    if (!check_segment_tables(first, count, n_segments, n_windows, R, max_frames, &longest, &cover))
        return DEMOD_BAD_ARG;
    const size_t dcap = hit_cap(max_frames, longest, R);
    if (!group_rows_ok(n_segments, dcap, true)) return DEMOD_BAD_ARG;
    const size_t work = demod_frames_segments_workspace_size(&st->cfg, n_segments, cover);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    const size_t N = frame_symbols, B = packed_row_bytes(N, demod_bits_per_symbol(st->cfg.k));
    const size_t n_rows = dcap * n_segments;
    const bool want_payload = payload && N && dcap, want_packed = packed && N && dcap;
    HIP_TRY(st->d_seg_work.reserve(work));  // bytes
    HIP_TRY(st->d_seg_first.reserve(n_segments));
    HIP_TRY(st->d_seg_count.reserve(n_segments));
    HIP_TRY(st->d_fsg_res.reserve(n_segments));
    HIP_TRY(st->d_fsg_hits.reserve(n_rows));
    HIP_TRY(st->h_fsg_hits.reserve(n_rows));
    if (want_payload) {
        HIP_TRY(st->d_fsg_payload.reserve(n_rows * N));
        HIP_TRY(st->h_fsg_payload.reserve(n_rows * N));
    }
    if (want_packed) {
        HIP_TRY(st->d_fsg_packed.reserve(n_rows * B));
        HIP_TRY(st->h_fsg_packed.reserve(n_rows * B));
    }
    int rc;
    if ((rc = upload_segment_tables(st, first, count, n_segments)) != DEMOD_OK) return rc;
    if ((rc = stage_and_detect(st, pcm, n_windows)) != DEMOD_OK) return rc;
    rc = demod_frames_segments_async(st, st->d_sym.p, st->d_mag.p, n_windows, st->d_seg_first.p,
                                     st->d_seg_count.p, n_segments, sync, sync_len, max_errors, N,
                                     dcap ? st->d_fsg_hits.p : nullptr,
                                     want_payload ? st->d_fsg_payload.p : nullptr,
                                     want_packed ? st->d_fsg_packed.p : nullptr, dcap, st->d_fsg_res.p,
                                     st->d_seg_work.p, work, st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(results, st->d_fsg_res.p, n_segments * sizeof(*results),
                           hipMemcpyDeviceToHost, st->stream));
    // the rows through pinned staging in the same pass, then each segment's
    // written rows to the caller's [S][max_frames]
    if (dcap) {
        HIP_TRY(hipMemcpyAsync(st->h_fsg_hits.p, st->d_fsg_hits.p, n_rows * sizeof(*hits),
                               hipMemcpyDeviceToHost, st->stream));
        if (want_payload)
            HIP_TRY(hipMemcpyAsync(st->h_fsg_payload.p, st->d_fsg_payload.p, n_rows * N,
                                   hipMemcpyDeviceToHost, st->stream));
        if (want_packed)
            HIP_TRY(hipMemcpyAsync(st->h_fsg_packed.p, st->d_fsg_packed.p, n_rows * B,
                                   hipMemcpyDeviceToHost, st->stream));
    }
    HIP_TRY(hipStreamSynchronize(st->stream));
    unsigned long long total = 0;
    for (size_t s = 0; s < n_segments; ++s) {
        const size_t nw = (size_t)results[s].n_written;
        if (nw) {
            std::memcpy(hits + s * max_frames, st->h_fsg_hits.p + s * dcap, nw * sizeof(*hits));
            if (want_payload)
                std::memcpy(payload + s * max_frames * N, st->h_fsg_payload.p + s * dcap * N, nw * N);
            if (want_packed)
                std::memcpy(packed + s * max_frames * B, st->h_fsg_packed.p + s * dcap * B, nw * B);
        }
        total += nw;
    }
    return (int)total;
}

}  // extern "C"
