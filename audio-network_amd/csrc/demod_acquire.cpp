// demod_acquire.cpp — the C ABI of everything downstream of the detector
// (include/demod.h): acquisition, the frame scan, their segmented forms, the
// frame check, the coded decode and the receiver's two stages (the receiver
// handle itself is demod_rx.cpp). Each stage has a workspace-size function,
// an *_async call on device memory and the caller's stream, and a synchronous
// wrapper that stages host or device samples, runs the detector (enqueue_batch,
// demod_api.cpp) and the stage on the handle's stream and copies the results.
#include <algorithm>
#include <cstring>

#include "demod_host.h"

using namespace fskd;

// R = n / hop when it divides and is at most DEMOD_MAX_PHASES, else 0 (n and
// hop are powers of two for every valid configuration, so R is one)
static uint32_t acquire_phases(const demod_cfg_t &c)
{
    if (c.hop == 0 || c.n % c.hop != 0) return 0;
    const uint32_t r = c.n / c.hop;
    return (r >= 1 && r <= DEMOD_MAX_PHASES && (r & (r - 1)) == 0) ? r : 0;
}

// The handle's R when the shape and the sync word are acceptable, else 0.
// whole: the batch is acquired as one stream and needs R windows (a segment
// with fewer is an outcome of the segmented call, not a refusal).
static uint32_t acquire_check(const demod_t *st, size_t n_windows, const uint8_t *sync,
                              size_t sync_len, uint32_t max_errors, bool whole = true)
{
    if (!st) return 0;
    const uint32_t R = acquire_phases(st->cfg);
    if (R == 0 || (whole && n_windows < R) || n_windows > 0x7FFFFFFF) return 0;
    if (sync_len > DEMOD_MAX_SYNC || (sync_len && (!sync || max_errors >= sync_len))) return 0;
    for (size_t i = 0; i < sync_len; ++i)
        if (sync[i] >= st->cfg.k) return 0;
    return R;
}

// The handle's R when a frame scan of these arguments is acceptable, else 0:
// what acquire_check refuses, no word, or a frame of 2^31 windows or more.
static uint32_t frames_check(const demod_t *st, size_t n_windows, const uint8_t *sync,
                             size_t sync_len, uint32_t max_errors, size_t frame_symbols,
                             size_t max_frames, bool whole = true)
{
    const uint32_t R = acquire_check(st, n_windows, sync, sync_len, max_errors, whole);
    if (R == 0 || sync_len == 0 || max_frames > 0x7FFFFFFF) return 0;
    if (frame_symbols > 0x7FFFFFFF || (sync_len + frame_symbols) * R > 0x7FFFFFFF) return 0;
    return R;
}

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
    return n_segments != 0 && n_segments <= DEMOD_MAX_SEGMENTS && ((uintptr_t)d_first & 7) == 0 &&
           ((uintptr_t)d_count & 3) == 0;
}

// Bytes of a packed row: N symbols of `bits` bits, MSB first, the last byte padded
static size_t packed_row_bytes(size_t N, size_t bits) { return (N * bits + 7) / 8; }

// Rows a synchronous wrapper keeps on the device for `windows` windows: the
// caller's cap, or every row there can be. Acquisition writes one symbol per R
// windows (n_out <= ceil(W / R)); complete hits are starts on one phase whose
// frame fits, so W / R + 1 bounds them too.
static size_t hit_cap(size_t cap, size_t windows, uint32_t R) { return std::min(cap, windows / R + 1); }

// The synchronous wrappers' first half, on st->stream: the batch's samples on
// the device (host samples are copied to st->d_in, a device pointer is read in
// place), then the detector into st->d_sym and st->d_mag.
static int stage_and_detect(demod_t *st, const int16_t *pcm, size_t n_windows)
{
    const size_t n_samples = (n_windows - 1) * st->cfg.hop + st->cfg.n;
    const bool din = is_device_ptr(pcm);
    int rc;
    if ((rc = ensure_dev(st, din ? 0 : n_samples, n_windows, true)) != DEMOD_OK) return rc;
    if (!din)
        HIP_TRY(hipMemcpyAsync(st->d_in.p, pcm, n_samples * sizeof(int16_t), hipMemcpyHostToDevice,
                               st->stream));
    rc = enqueue_batch(st, din ? pcm : st->d_in.p, n_windows, st->d_sym.p, st->d_mag.p, st->stream);
    return rc < 0 ? rc : DEMOD_OK;
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
    if (!d_symbols || !d_mags || !d_result || !d_work) return DEMOD_BAD_ARG;
    const uint32_t R = acquire_check(st, n_windows, sync, sync_len, max_errors);
    if (R == 0) return DEMOD_BAD_ARG;
    if ((cap && !d_out) || ((uintptr_t)d_result & 7) != 0 || ((uintptr_t)d_work & 7) != 0)
        return DEMOD_BAD_ARG;
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
    if (!pcm || !result || (cap && !out) || ((uintptr_t)pcm & 15) != 0) return DEMOD_BAD_ARG;
    const uint32_t R = acquire_check(st, n_windows, sync, sync_len, max_errors);
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
    if (!d_symbols || !d_mags || !d_results || !d_work || !d_first || !d_count) return DEMOD_BAD_ARG;
    const uint32_t R = acquire_check(st, n_windows, sync, sync_len, max_errors, false);
    if (R == 0 || !seg_call_ok(n_segments, d_first, d_count)) return DEMOD_BAD_ARG;
    if ((cap && !d_out) || ((uintptr_t)d_results & 7) != 0 || ((uintptr_t)d_work & 7) != 0)
        return DEMOD_BAD_ARG;
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
    if (!pcm || !results || !first || !count || (cap && !out) || ((uintptr_t)pcm & 15) != 0)
        return DEMOD_BAD_ARG;
    const uint32_t R = acquire_check(st, n_windows, sync, sync_len, max_errors);
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
    if (!d_symbols || !d_mags || !d_result || !d_work) return DEMOD_BAD_ARG;
    const uint32_t R = frames_check(st, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames);
    if (R == 0) return DEMOD_BAD_ARG;
    if ((max_frames && !d_hits) || ((uintptr_t)d_hits & 7) != 0 || ((uintptr_t)d_result & 7) != 0 ||
        ((uintptr_t)d_work & 7) != 0)
        return DEMOD_BAD_ARG;
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
    if (!pcm || !result || (max_frames && !hits) || ((uintptr_t)pcm & 15) != 0) return DEMOD_BAD_ARG;
    const uint32_t R = frames_check(st, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames);
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
    if (!d_symbols || !d_mags || !d_results || !d_work || !d_first || !d_count) return DEMOD_BAD_ARG;
    const uint32_t R =
        frames_check(st, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames, false);
    if (R == 0 || !seg_call_ok(n_segments, d_first, d_count)) return DEMOD_BAD_ARG;
    if ((unsigned long long)n_segments * max_frames > 0x7FFFFFFFull) return DEMOD_BAD_ARG;
    if ((max_frames && !d_hits) || ((uintptr_t)d_hits & 7) != 0 || ((uintptr_t)d_results & 7) != 0 ||
        ((uintptr_t)d_work & 7) != 0)
        return DEMOD_BAD_ARG;
    const size_t need = demod_frames_segments_workspace_size(&st->cfg, n_segments, n_windows);
    if (need == 0 || work_bytes < need) return DEMOD_BAD_ARG;
    const size_t budget = std::min<size_t>(
        frames_seg_budget(work_bytes - acquire_seg_header_bytes(n_segments), R), 0xFFFFFFFFu);
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
    if (!pcm || !results || !first || !count || (max_frames && !hits) || ((uintptr_t)pcm & 15) != 0)
        return DEMOD_BAD_ARG;
    const uint32_t R = frames_check(st, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames);
    if (R == 0 || n_segments == 0 || n_segments > DEMOD_MAX_SEGMENTS) return DEMOD_BAD_ARG;
    size_t longest, cover;
    if (!check_segment_tables(first, count, n_segments, n_windows, R, max_frames, &longest, &cover))
        return DEMOD_BAD_ARG;
    const size_t dcap = hit_cap(max_frames, longest, R);
    if ((unsigned long long)n_segments * dcap > 0x7FFFFFFFull) return DEMOD_BAD_ARG;
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

// ---- checked frames (frames_check.hip) ---------------------------------------

// St of rows of C = N bits soft values in a valid mode (C < 2^33; a mapped mode's beyond 2^32 - 1: 0)
static size_t fec_row_steps(unsigned fec, size_t C)
{
    if (!fec_mode_mapped(fec)) return C / 2;
    return C > 0xFFFFFFFFu ? 0 : fec_steps_within(fec, fec_usable_bits(fec, (unsigned)C));
}

// Fills what the shape decides (row width, max_len, the CRC's constants, R,
// bits, L); false for what demod_frames_check_async refuses about it.
static bool frames_check_shape(const demod_cfg_t &cfg, size_t n_groups, size_t max_frames, size_t sync_len,
                               size_t frame_symbols, int len_bytes, int crc, FramesCheckParams &p,
                               int fec = 0)
{
    const uint32_t R = acquire_phases(cfg);
    if (R == 0 || n_groups == 0 || n_groups > DEMOD_MAX_SEGMENTS || max_frames == 0) return false;
    if (max_frames > 0x7FFFFFFF || (unsigned long long)n_groups * max_frames > 0x7FFFFFFFull) return false;
    if (sync_len == 0 || sync_len > DEMOD_MAX_SYNC || (len_bytes != 1 && len_bytes != 2)) return false;
    if (crc != DEMOD_CRC16_CCITT_FALSE && crc != DEMOD_CRC32_MPEG2) return false;
    const size_t bits = (size_t)demod_bits_per_symbol(cfg.k);
    const size_t c = crc == DEMOD_CRC16_CCITT_FALSE ? 2 : 4, h = (size_t)len_bytes;
    if (frame_symbols > 0x7FFFFFFF) return false;
    size_t B = packed_row_bytes(frame_symbols, bits);
    if (fec && !rs_mode_valid((unsigned)fec)) return false;
    const unsigned conv = rs_mode_conv((unsigned)fec), P = rs_parity((unsigned)fec);
    if (conv) {
        // coded rows: the mode's St steps (fec_map.h) decode to Bd = (St - 6) / 8 bytes
        if (cfg.k != (1u << bits)) return false;
        const size_t St = fec_row_steps(conv, frame_symbols * bits);
        if (St < 8 * h + DEMOD_FEC_DEPTH) return false;
        B = (St - 6) / 8;
        p.fec_depth = DEMOD_FEC_DEPTH;
        p.fec = (int)conv;
    }
    // max_len: the greatest len whose frame fits the row; with an outer code its n' bytes (rs_ops.h)
    const long long M = P ? rs_max_len((unsigned)B, (unsigned)h, (unsigned)c, P) : (long long)B - (long long)(h + c);
    if (M < 0 || M > DEMOD_MAX_FRAME_PAYLOAD) return false;
    p.parity = (int)P;
    p.n_groups = (unsigned)n_groups;
    p.max_frames = (unsigned)max_frames;
    p.row_bytes = (unsigned)B;
    p.max_len = (unsigned)M;
    p.len_bytes = len_bytes;
    p.crc_bytes = (int)c;
    p.poly = c == 2 ? 0x1021u << 16 : 0x04C11DB7u;
    p.init = c == 2 ? 0xFFFFu << 16 : 0xFFFFFFFFu;
    // x^8, then its squares mod P (Horner over the square's own coefficients, highest first)
    static_assert(DEMOD_MAX_FRAME_PAYLOAD + 2 < (1 << kCrcPowBits), "bytes after a lane's chunk");
    const int width = 8 * (int)c;
    p.xpow8[0] = 1u << (32 - width + 8);
    for (int j = 1; j < kCrcPowBits; ++j) {
        const uint32_t a = p.xpow8[j - 1];
        uint32_t r = 0, b = a;
        for (int i = 0; i < width; ++i, b <<= 1)
            r = (r << 1) ^ ((r >> 31) ? p.poly : 0u) ^ ((b >> 31) ? a : 0u);
        p.xpow8[j] = r;
    }
    p.bits = (int)bits;
    p.phases = (int)R;
    p.sync_len = (int)sync_len;
    return true;
}

static bool frames_check_shape(const demod_t *st, size_t n_groups, size_t max_frames, size_t sync_len,
                               size_t frame_symbols, int len_bytes, int crc, FramesCheckParams &p,
                               int fec = 0)
{
    return st && frames_check_shape(st->cfg, n_groups, max_frames, sync_len, frame_symbols, len_bytes, crc, p, fec);
}

// fec 0: the scan's packed rows; else decoded rows (the coded entry has refused fec 0)
static int frames_check_enqueue(demod_t *st, const demod_frame_hit_t *d_hits, const uint8_t *d_packed,
                                const demod_frames_result_t *d_results, size_t n_groups,
                                size_t max_frames, size_t sync_len, size_t frame_symbols, int len_bytes,
                                int crc, int fec, demod_frame_check_t *d_check, uint32_t *d_kept,
                                uint8_t *d_body, demod_frames_check_result_t *d_summary, void *stream)
{
    if (!st || !d_hits || !d_packed || !d_results || !d_check || !d_kept || !d_summary) return DEMOD_BAD_ARG;
    if (((uintptr_t)d_hits & 7) != 0 || ((uintptr_t)d_results & 7) != 0 || ((uintptr_t)d_summary & 7) != 0 ||
        ((uintptr_t)d_check & 3) != 0 || ((uintptr_t)d_kept & 3) != 0)
        return DEMOD_BAD_ARG;
    FramesCheckParams p;
    std::memset(&p, 0, sizeof(p));
    if (!frames_check_shape(st, n_groups, max_frames, sync_len, frame_symbols, len_bytes, crc, p, fec))
        return DEMOD_BAD_ARG;
    p.hits = d_hits;
    p.packed = d_packed;
    p.res = d_results;
    p.check = d_check;
    p.kept = d_kept;
    p.body = d_body;
    p.summary = d_summary;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_frames_check(p, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_frames_check_async(demod_t *st, const demod_frame_hit_t *d_hits, const uint8_t *d_packed,
                             const demod_frames_result_t *d_results, size_t n_groups,
                             size_t max_frames, size_t sync_len, size_t frame_symbols, int len_bytes,
                             int crc, demod_frame_check_t *d_check, uint32_t *d_kept, uint8_t *d_body,
                             demod_frames_check_result_t *d_summary, void *stream)
{
    return frames_check_enqueue(st, d_hits, d_packed, d_results, n_groups, max_frames, sync_len,
                                frame_symbols, len_bytes, crc, 0, d_check, d_kept, d_body, d_summary, stream);
}

// ---- coded frames (frames_fec.hip) -------------------------------------------

size_t demod_frames_decode_workspace_size(const demod_cfg_t *cfg, size_t n_groups, size_t max_frames,
                                          size_t frame_symbols)
{
    return demod_fec_decode_workspace_size(cfg, n_groups, max_frames, frame_symbols, DEMOD_FEC_CONV_K7);
}

size_t demod_fec_decode_workspace_size(const demod_cfg_t *cfg, size_t n_groups, size_t max_frames,
                                       size_t frame_symbols, int fec)
{
    if (!rs_mode_valid((unsigned)fec) || !rs_mode_conv((unsigned)fec)) return 0;
    fec = (int)rs_mode_conv((unsigned)fec);   // a parity flag does not change the trellis's workspace
    if (validate_cfg(cfg) != DEMOD_OK || cfg->k < 2 || (cfg->k & (cfg->k - 1)) != 0) return 0;
    if (n_groups == 0 || n_groups > DEMOD_MAX_SEGMENTS || max_frames == 0 || max_frames > 0x7FFFFFFF) return 0;
    if ((unsigned long long)n_groups * max_frames > 0x7FFFFFFFull) return 0;
    if (frame_symbols == 0 || frame_symbols > 0x7FFFFFFF) return 0;
    const size_t St = fec_row_steps((unsigned)fec, frame_symbols * (size_t)demod_bits_per_symbol(cfg->k));
    return n_groups * (size_t)fec_waves_per_group((unsigned)n_groups, (unsigned)max_frames) * St * 8;
}

int demod_frames_decode_async(demod_t *st, const demod_frame_hit_t *d_hits, const float *d_mags,
                              size_t n_windows, const uint64_t *d_first,
                              const demod_frames_result_t *d_results, size_t n_groups,
                              size_t max_frames, size_t sync_len, size_t frame_symbols, int len_bytes,
                              int crc, int fec, uint8_t *d_rows, demod_frame_decode_t *d_decode,
                              void *d_work, size_t work_bytes, void *stream)
{
    if (!st || !d_hits || !d_mags || !d_results || !d_rows || !d_decode || !d_work) return DEMOD_BAD_ARG;
    if (((uintptr_t)d_hits & 7) != 0 || ((uintptr_t)d_results & 7) != 0 || ((uintptr_t)d_work & 7) != 0 ||
        ((uintptr_t)d_first & 7) != 0 || ((uintptr_t)d_decode & 3) != 0)
        return DEMOD_BAD_ARG;
    if (!rs_mode_valid((unsigned)fec) || !rs_mode_conv((unsigned)fec) || n_windows > 0x7FFFFFFF)
        return DEMOD_BAD_ARG;
    const int conv = (int)rs_mode_conv((unsigned)fec);   // the trellis's mode; the parity flag sizes the frame
    FramesCheckParams q;   // the shape the coded check will see: the same refusals
    std::memset(&q, 0, sizeof(q));
    if (!frames_check_shape(st, n_groups, max_frames, sync_len, frame_symbols, len_bytes, crc, q, fec))
        return DEMOD_BAD_ARG;
    if ((sync_len + frame_symbols) * (size_t)q.phases > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    const size_t need = demod_fec_decode_workspace_size(&st->cfg, n_groups, max_frames, frame_symbols, conv);
    if (need == 0 || work_bytes < need) return DEMOD_BAD_ARG;
    FramesFecParams p;
    std::memset(&p, 0, sizeof(p));
    p.hits = d_hits;
    p.mag = d_mags;
    p.first = reinterpret_cast<const unsigned long long *>(d_first);
    p.res = d_results;
    p.n_windows = (unsigned)n_windows;
    p.n_groups = q.n_groups;
    p.max_frames = q.max_frames;
    p.frame_symbols = (unsigned)frame_symbols;
    p.steps = (unsigned)fec_row_steps((unsigned)conv, frame_symbols * (size_t)q.bits);
    p.fec = (unsigned)conv;
    p.parity = (unsigned)q.parity;
    p.row_bytes = q.row_bytes;
    p.max_len = q.max_len;
    p.len_bytes = q.len_bytes;
    p.crc_bytes = q.crc_bytes;
    p.k = (int)st->cfg.k;
    p.bits = q.bits;
    p.phases = q.phases;
    p.sync_len = q.sync_len;
    p.rows = d_rows;
    p.decode = d_decode;
    p.work = static_cast<unsigned long long *>(d_work);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_frames_decode(p, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_frames_check_coded_async(demod_t *st, const demod_frame_hit_t *d_hits, const uint8_t *d_rows,
                                   const demod_frames_result_t *d_results, size_t n_groups,
                                   size_t max_frames, size_t sync_len, size_t frame_symbols,
                                   int len_bytes, int crc, int fec, demod_frame_check_t *d_check,
                                   uint32_t *d_kept, uint8_t *d_body,
                                   demod_frames_check_result_t *d_summary, void *stream)
{
    if (!rs_mode_valid((unsigned)fec)) return DEMOD_BAD_ARG;
    return frames_check_enqueue(st, d_hits, d_rows, d_results, n_groups, max_frames, sync_len,
                                frame_symbols, len_bytes, crc, fec, d_check, d_kept, d_body, d_summary, stream);
}

int demod_frames_rs_async(demod_t *st, uint8_t *d_rows, const demod_frames_result_t *d_results,
                          size_t n_groups, size_t max_frames, size_t frame_symbols, int len_bytes, int crc,
                          int fec, demod_frame_rs_t *d_rs, void *stream)
{
    if (!st || !d_rows || !d_results || !d_rs) return DEMOD_BAD_ARG;
    if (((uintptr_t)d_results & 7) != 0 || ((uintptr_t)d_rs & 3) != 0) return DEMOD_BAD_ARG;
    if (!rs_mode_valid((unsigned)fec) || !rs_parity((unsigned)fec)) return DEMOD_BAD_ARG;
    FramesCheckParams q;   // the shape the coded check will see: the same refusals (it has no word here)
    std::memset(&q, 0, sizeof(q));
    if (!frames_check_shape(st, n_groups, max_frames, 1, frame_symbols, len_bytes, crc, q, fec))
        return DEMOD_BAD_ARG;
    FramesRsParams p;
    std::memset(&p, 0, sizeof(p));
    p.rows = d_rows;
    p.res = d_results;
    p.n_groups = q.n_groups;
    p.max_frames = q.max_frames;
    p.row_bytes = q.row_bytes;
    p.max_len = q.max_len;
    p.len_bytes = q.len_bytes;
    p.crc_bytes = q.crc_bytes;
    p.parity = q.parity;
    p.rs = d_rs;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_frames_rs(p, (hipStream_t)stream));
    return DEMOD_OK;
}

// demod_frames_checked (fec 0: the scan's packed rows) and demod_frames_coded
static int frames_checked_run(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                              size_t sync_len, uint32_t max_errors, size_t frame_symbols, int len_bytes,
                              int crc, int fec, demod_frame_hit_t *hits, uint32_t *lengths, uint8_t *body,
                              size_t max_frames, demod_frames_result_t *result,
                              demod_frames_check_result_t *summary)
{
    if (!pcm || !result || !summary || !hits || !lengths || ((uintptr_t)pcm & 15) != 0) return DEMOD_BAD_ARG;
    const uint32_t R = frames_check(st, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames);
    if (R == 0) return DEMOD_BAD_ARG;   // before the detector runs
    const size_t dcap = hit_cap(max_frames, n_windows, R);
    FramesCheckParams p;
    std::memset(&p, 0, sizeof(p));
    if (!frames_check_shape(st, 1, dcap, sync_len, frame_symbols, len_bytes, crc, p, fec)) return DEMOD_BAD_ARG;
    // conv: the trellis's mode or 0 (the scan's packed rows); p.parity: the outer code's stage before the check
    const int conv = (int)rs_mode_conv((unsigned)fec);
    const size_t fec_work = conv ? demod_fec_decode_workspace_size(&st->cfg, 1, dcap, frame_symbols, conv) : 0;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    const size_t N = frame_symbols, B = p.row_bytes, M = p.max_len;
    const bool want_body = body && M;
    const size_t work = demod_frames_workspace_size(&st->cfg, n_windows);
    HIP_TRY(st->d_frm_work.reserve(work));  // bytes
    HIP_TRY(st->d_frm_res.reserve(1));
    HIP_TRY(st->d_frm_hits.reserve(dcap));
    if (conv) {
        HIP_TRY(st->d_fec_rows.reserve(dcap * B));
        HIP_TRY(st->d_fec_decode.reserve(dcap));
        HIP_TRY(st->d_fec_work.reserve(fec_work));  // bytes
    } else {
        HIP_TRY(st->d_frm_packed.reserve(dcap * B));
    }
    if (p.parity) HIP_TRY(st->d_rs.reserve(dcap));
    HIP_TRY(st->d_chk_check.reserve(dcap));
    HIP_TRY(st->d_chk_kept.reserve(dcap));
    HIP_TRY(st->d_chk_sum.reserve(1));
    HIP_TRY(st->d_chk_hits.reserve(dcap));
    HIP_TRY(st->d_chk_len.reserve(dcap));
    if (want_body) HIP_TRY(st->d_chk_body.reserve(dcap * M));
    int rc;
    if ((rc = stage_and_detect(st, pcm, n_windows)) != DEMOD_OK) return rc;
    rc = demod_frames_async(st, st->d_sym.p, st->d_mag.p, n_windows, sync, sync_len, max_errors, N,
                            st->d_frm_hits.p, nullptr, conv ? nullptr : st->d_frm_packed.p, dcap,
                            st->d_frm_res.p, st->d_frm_work.p, work, st->stream);
    if (rc < 0) return rc;
    uint8_t *rows = conv ? st->d_fec_rows.p : st->d_frm_packed.p;
    if (conv) {
        rc = demod_frames_decode_async(st, st->d_frm_hits.p, st->d_mag.p, n_windows, nullptr, st->d_frm_res.p,
                                       1, dcap, sync_len, N, len_bytes, crc, fec, st->d_fec_rows.p,
                                       st->d_fec_decode.p, st->d_fec_work.p, fec_work, st->stream);
        if (rc < 0) return rc;
    }
    if (p.parity) {
        rc = demod_frames_rs_async(st, rows, st->d_frm_res.p, 1, dcap, N, len_bytes, crc, fec, st->d_rs.p,
                                   st->stream);
        if (rc < 0) return rc;
    }
    rc = frames_check_enqueue(st, st->d_frm_hits.p, rows,
                              st->d_frm_res.p, 1, dcap, sync_len, N, len_bytes, crc, fec, st->d_chk_check.p,
                              st->d_chk_kept.p, want_body ? st->d_chk_body.p : nullptr, st->d_chk_sum.p,
                              st->stream);
    if (rc < 0) return rc;
    // the kept rows' hits and lengths side by side, so that only they cross to the host
    HIP_TRY(launch_frames_kept_rows(st->d_frm_hits.p, st->d_chk_check.p, st->d_chk_kept.p, st->d_chk_sum.p,
                                    (unsigned)dcap, st->d_chk_hits.p, st->d_chk_len.p, st->stream));
    HIP_TRY(hipMemcpyAsync(result, st->d_frm_res.p, sizeof(*result), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipMemcpyAsync(summary, st->d_chk_sum.p, sizeof(*summary), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    const size_t nk = (size_t)summary->n_kept;
    if (nk) {
        HIP_TRY(hipMemcpy(hits, st->d_chk_hits.p, nk * sizeof(*hits), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(lengths, st->d_chk_len.p, nk * sizeof(*lengths), hipMemcpyDeviceToHost));
        if (want_body) {
            // a body row holds its frame's bytes alone: the rest of the caller's row is left as it is
            st->h_chk_body.resize(nk * M);
            HIP_TRY(hipMemcpy(st->h_chk_body.data(), st->d_chk_body.p, nk * M, hipMemcpyDeviceToHost));
            for (size_t r = 0; r < nk; ++r)
                std::memcpy(body + r * M, st->h_chk_body.data() + r * M, lengths[r]);
        }
    }
    return (int)nk;
}

int demod_frames_checked(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                         size_t sync_len, uint32_t max_errors, size_t frame_symbols, int len_bytes,
                         int crc, demod_frame_hit_t *hits, uint32_t *lengths, uint8_t *body,
                         size_t max_frames, demod_frames_result_t *result,
                         demod_frames_check_result_t *summary)
{
    return frames_checked_run(st, pcm, n_windows, sync, sync_len, max_errors, frame_symbols, len_bytes, crc,
                              0, hits, lengths, body, max_frames, result, summary);
}

int demod_frames_coded(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                       size_t sync_len, uint32_t max_errors, size_t frame_symbols, int len_bytes,
                       int crc, int fec, demod_frame_hit_t *hits, uint32_t *lengths, uint8_t *body,
                       size_t max_frames, demod_frames_result_t *result,
                       demod_frames_check_result_t *summary)
{
    if (!rs_mode_valid((unsigned)fec)) return DEMOD_BAD_ARG;
    return frames_checked_run(st, pcm, n_windows, sync, sync_len, max_errors, frame_symbols, len_bytes, crc,
                              fec, hits, lengths, body, max_frames, result, summary);
}

// ---- receiver stages (frames_carry.hip) ----------------------------------------

int demod_rx_sizes(const demod_cfg_t *cfg, const demod_rx_cfg_t *rxcfg, size_t n_streams,
                   demod_rx_sizes_t *out)
{
    if (!rxcfg || !out || validate_cfg(cfg) != DEMOD_OK) return DEMOD_BAD_ARG;
    const demod_rx_cfg_t &x = *rxcfg;
    const size_t S = n_streams, L = x.sync_len, N = x.frame_symbols, C = x.ring_windows;
    // the scan's refusals (acquire_check and frames_check, on the configuration)
    const uint32_t R = acquire_phases(*cfg);
    if (R == 0 || L == 0 || L > DEMOD_MAX_SYNC || x.max_errors >= L) return DEMOD_BAD_ARG;
    for (size_t i = 0; i < L; ++i)
        if (x.sync[i] >= cfg->k) return DEMOD_BAD_ARG;
    if (N > 0x7FFFFFFF || (L + N) * R > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    if (x.fec != 0 && !rs_mode_valid(x.fec)) return DEMOD_BAD_ARG;
    const int conv = (int)rs_mode_conv(x.fec);   // the trellis's mode, or 0
    // the check's (or the decode's and the coded check's): S, max_frames, the row shape
    FramesCheckParams p;
    std::memset(&p, 0, sizeof(p));
    if (!frames_check_shape(*cfg, S, x.max_frames, L, N, (int)x.len_bytes, (int)x.crc, p, (int)x.fec))
        return DEMOD_BAD_ARG;
    if (C < 2 * (L + N) * R || C >= ((size_t)1 << 31) / S || S * C > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    const size_t rows = S * x.max_frames;
    out->max_len = p.max_len;
    out->row_bytes = p.row_bytes;
    out->ring_sym_bytes = S * C;
    out->ring_mag_bytes = S * C * cfg->k * sizeof(float);
    out->scan_work_bytes = demod_frames_segments_workspace_size(cfg, S, S * C);
    out->decode_work_bytes = conv ? demod_fec_decode_workspace_size(cfg, S, x.max_frames, N, conv) : 0;
    out->collect_work_bytes = demod_rx_collect_workspace_size(cfg, S);
    out->frames_bytes = rows * sizeof(demod_rx_frame_t);
    out->bodies_bytes = rows * p.max_len;
    if (out->scan_work_bytes == 0 || (conv && out->decode_work_bytes == 0)) return DEMOD_BAD_ARG;
    return DEMOD_OK;
}

int demod_rx_advance_async(demod_t *st, demod_rx_stream_state_t *d_state, const uint8_t *d_ring_sym_in,
                           const float *d_ring_mag_in, const uint8_t *d_new_sym, const float *d_new_mag,
                           size_t n_new_windows, const uint64_t *d_new_first,
                           const uint32_t *d_new_count, size_t n_streams, size_t ring_windows,
                           uint8_t *d_ring_sym_out, float *d_ring_mag_out, uint64_t *d_first,
                           uint32_t *d_count, void *stream)
{
    if (!st || !d_state || !d_ring_sym_in || !d_ring_mag_in || !d_new_sym || !d_new_mag || !d_new_first ||
        !d_new_count || !d_ring_sym_out || !d_ring_mag_out || !d_first || !d_count)
        return DEMOD_BAD_ARG;
    if (d_ring_sym_in == d_ring_sym_out || d_ring_mag_in == d_ring_mag_out) return DEMOD_BAD_ARG;
    if (n_streams == 0 || n_streams > DEMOD_MAX_SEGMENTS || ring_windows == 0 || ring_windows > 0x7FFFFFFF ||
        n_streams * ring_windows > 0x7FFFFFFF || n_new_windows > 0x7FFFFFFF)
        return DEMOD_BAD_ARG;
    if (((uintptr_t)d_state & 7) != 0 || ((uintptr_t)d_new_first & 7) != 0 || ((uintptr_t)d_first & 7) != 0 ||
        ((uintptr_t)d_new_count & 3) != 0 || ((uintptr_t)d_count & 3) != 0 ||
        ((uintptr_t)d_ring_mag_in & 3) != 0 || ((uintptr_t)d_ring_mag_out & 3) != 0 ||
        ((uintptr_t)d_new_mag & 3) != 0)
        return DEMOD_BAD_ARG;
    RxAdvanceParams p;
    std::memset(&p, 0, sizeof(p));
    p.state = d_state;
    p.ring_sym_in = d_ring_sym_in;
    p.ring_mag_in = d_ring_mag_in;
    p.new_sym = d_new_sym;
    p.new_mag = d_new_mag;
    p.new_first = reinterpret_cast<const unsigned long long *>(d_new_first);
    p.new_count = d_new_count;
    p.n_new = n_new_windows;
    p.n_streams = (unsigned)n_streams;
    p.ring = (unsigned)ring_windows;
    p.k = (int)st->cfg.k;
    p.ring_sym_out = d_ring_sym_out;
    p.ring_mag_out = d_ring_mag_out;
    p.seg_first = reinterpret_cast<unsigned long long *>(d_first);
    p.seg_count = d_count;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_rx_advance(p, (hipStream_t)stream));
    return DEMOD_OK;
}

size_t demod_rx_collect_workspace_size(const demod_cfg_t *cfg, size_t n_streams)
{
    if (validate_cfg(cfg) != DEMOD_OK || n_streams == 0 || n_streams > DEMOD_MAX_SEGMENTS) return 0;
    return rx_collect_work_bytes(n_streams);
}

int demod_rx_collect_async(demod_t *st, demod_rx_stream_state_t *d_state, const demod_frame_hit_t *d_hits,
                           const demod_frames_result_t *d_results, const demod_frame_check_t *d_check,
                           const uint32_t *d_kept, const uint8_t *d_body,
                           const demod_frames_check_result_t *d_check_summary, size_t n_streams,
                           size_t max_frames, size_t sync_len, size_t frame_symbols, int len_bytes,
                           int crc, int fec, demod_rx_frame_t *d_frames, uint8_t *d_bodies,
                           demod_rx_summary_t *d_summary, void *d_work, size_t work_bytes, void *stream)
{
    if (!st || !d_state || !d_hits || !d_results || !d_check || !d_kept || !d_check_summary || !d_frames ||
        !d_summary || !d_work)
        return DEMOD_BAD_ARG;
    if (((uintptr_t)d_state & 7) != 0 || ((uintptr_t)d_hits & 7) != 0 || ((uintptr_t)d_results & 7) != 0 ||
        ((uintptr_t)d_check_summary & 7) != 0 || ((uintptr_t)d_frames & 7) != 0 ||
        ((uintptr_t)d_summary & 7) != 0 || ((uintptr_t)d_work & 7) != 0 || ((uintptr_t)d_check & 3) != 0 ||
        ((uintptr_t)d_kept & 3) != 0)
        return DEMOD_BAD_ARG;
    if (fec != 0 && !rs_mode_valid((unsigned)fec)) return DEMOD_BAD_ARG;
    FramesCheckParams q;   // the shape the check saw: the same refusals, the same span
    std::memset(&q, 0, sizeof(q));
    if (!frames_check_shape(st, n_streams, max_frames, sync_len, frame_symbols, len_bytes, crc, q, fec))
        return DEMOD_BAD_ARG;
    if (q.max_len && (!d_body || !d_bodies)) return DEMOD_BAD_ARG;
    const size_t need = demod_rx_collect_workspace_size(&st->cfg, n_streams);
    if (need == 0 || work_bytes < need) return DEMOD_BAD_ARG;
    RxCollectParams p;
    std::memset(&p, 0, sizeof(p));
    p.state = d_state;
    p.hits = d_hits;
    p.res = d_results;
    p.check = d_check;
    p.kept = d_kept;
    p.body = d_body;
    p.chk_sum = d_check_summary;
    p.n_streams = q.n_groups;
    p.max_frames = q.max_frames;
    p.max_len = q.max_len;
    p.len_bytes = q.len_bytes;
    p.crc_bytes = q.crc_bytes;
    p.bits = q.bits;
    p.phases = q.phases;
    p.sync_len = q.sync_len;
    p.fec_depth = q.fec_depth;
    p.fec = q.fec;
    p.parity = q.parity;
    p.frames = d_frames;
    p.bodies = d_bodies;
    p.summary = d_summary;
    p.w_hold = static_cast<unsigned long long *>(d_work);
    p.w_bytes = p.w_hold + n_streams;
    p.w_cnt = reinterpret_cast<unsigned *>(p.w_bytes + n_streams);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_rx_collect(p, (hipStream_t)stream));
    return DEMOD_OK;
}

}  // extern "C"
