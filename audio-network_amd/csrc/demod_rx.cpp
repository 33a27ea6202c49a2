// demod_rx.cpp — the receiver (include/demod.h "receiver"): live streams in,
// checked frames out. The sizes and the two device stages' entry points
// (frames_carry.hip), and the handle. It owns a demod_streams_t for the sample
// side of a push (carries, lead-in, staging: demod_streams.cpp's own functions)
// and, on the device, two [S][C] rings of detector outputs, the stages' buffers
// and one output block; a push is one copy in, the stages' launches on the
// detector handle's stream (the *_async entries of demod_acquire.cpp, demod_frames.cpp
// and this file, as any caller would chain them) and one copy out.
#include <cstring>
#include <new>
#include <vector>

#include "demod_host.h"

using namespace fskd;

extern "C" {

// ---- receiver stages (frames_carry.hip) ----------------------------------------

int demod_rx_sizes(const demod_cfg_t *cfg, const demod_rx_cfg_t *rxcfg, size_t n_streams,
                   demod_rx_sizes_t *out)
{
    if (!rxcfg || !out || validate_cfg(cfg) != DEMOD_OK) return DEMOD_BAD_ARG;
    const demod_rx_cfg_t &x = *rxcfg;
    const size_t S = n_streams, L = x.sync_len, N = x.frame_symbols, C = x.ring_windows;
    // the segmented scan's refusals (the ring's windows are refused below)
    const uint32_t R = frames_args(*cfg, 0, x.sync, L, x.max_errors, N, x.max_frames, false);
    if (R == 0) return DEMOD_BAD_ARG;
    // the check's (or the decode's and the coded check's): S, max_frames, the row shape
    frame_shape s;
    // (a level of "erasure decoding" is the receiver's own: the row's shape is the mode's without it)
    if (x.fec && !rs_erase_mode_valid(x.fec)) return DEMOD_BAD_ARG;
    if (!stage_shape(*cfg, S, x.max_frames, L, N, (int)x.len_bytes, (int)x.crc, (int)rs_erase_strip(x.fec), s))
        return DEMOD_BAD_ARG;
    unsigned mask_row = 0;   // with a level: what the producer will ask of every push
    if (rs_erase_level(x.fec) && (!erasures_shape(*cfg, S, x.max_frames, L, N, mask_row) || mask_row != s.row_bytes))
        return DEMOD_BAD_ARG;
    if (C < 2 * (L + N) * R || C >= ((size_t)1 << 31) / S || S * C > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    const size_t rows = S * x.max_frames;
    out->max_len = s.max_len;
    out->row_bytes = s.row_bytes;
    out->ring_sym_bytes = S * C;
    out->ring_mag_bytes = S * C * cfg->k * sizeof(float);
    out->scan_work_bytes = demod_frames_segments_workspace_size(cfg, S, S * C);
    out->decode_work_bytes = s.fec ? demod_fec_decode_workspace_size(cfg, S, x.max_frames, N, s.fec) : 0;
    out->collect_work_bytes = demod_rx_collect_workspace_size(cfg, S);
    out->frames_bytes = rows * sizeof(demod_rx_frame_t);
    out->bodies_bytes = rows * s.max_len;
    if (out->scan_work_bytes == 0 || (s.fec && out->decode_work_bytes == 0)) return DEMOD_BAD_ARG;
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
    if (!aligned8(d_state, d_new_first, d_first) ||
        !aligned4(d_new_count, d_count, d_ring_mag_in, d_ring_mag_out, d_new_mag))
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
    if (!aligned8(d_state, d_hits, d_results, d_check_summary, d_frames, d_summary, d_work) ||
        !aligned4(d_check, d_kept))
        return DEMOD_BAD_ARG;
    frame_shape s;   // the shape the check saw: the same refusals, the same span
    const uint32_t R = stage_shape(st->cfg, n_streams, max_frames, sync_len, frame_symbols, len_bytes, crc, fec, s);
    if (R == 0) return DEMOD_BAD_ARG;
    if (s.max_len && (!d_body || !d_bodies)) return DEMOD_BAD_ARG;
    const size_t need = demod_rx_collect_workspace_size(&st->cfg, n_streams);
    if (need == 0 || work_bytes < need) return DEMOD_BAD_ARG;
    RxCollectParams p;
    std::memset(&p, 0, sizeof(p));
    fill_shape_fields(p, s, max_frames, R, sync_len);
    p.n_streams = (unsigned)n_streams;
    p.fec_depth = s.fec_depth;
    p.state = d_state;
    p.hits = d_hits;
    p.res = d_results;
    p.check = d_check;
    p.kept = d_kept;
    p.body = d_body;
    p.chk_sum = d_check_summary;
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

// ---- the handle ----------------------------------------------------------------

struct demod_rx {
    demod_cfg_t cfg;
    demod_rx_cfg_t rx;
    demod_rx_sizes_t sz;
    size_t S = 0;
    demod_streams_t *ms = nullptr;        // sample carries, lead-in, staging, the detector handle
    int cur = 0;                          // the ring that holds X
    DevBuf<uint8_t> ring_sym[2];          // [S][C]
    DevBuf<float> ring_mag[2];            // [S][C][K]
    DevBuf<uint64_t> d_first;             // the scan's tables, written by advance
    DevBuf<uint32_t> d_count;
    DevBuf<unsigned char> d_scan_work, d_fec_work, d_col_work;
    DevBuf<demod_frame_hit_t> d_hits;     // [S][max_frames]
    DevBuf<demod_frames_result_t> d_res;  // [S]
    DevBuf<uint8_t> d_rows;               // [S][max_frames][row_bytes]: packed, or decoded
    DevBuf<demod_frame_decode_t> d_decode;
    DevBuf<demod_frame_rs_t> d_rs;        // with a parity flag: the outer code's records
    DevBuf<uint64_t> d_erase;             // with a level: the rows' erasure masks and the decoder's second records
    DevBuf<demod_frame_erase_t> d_erec;
    DevBuf<demod_frame_check_t> d_check;
    DevBuf<uint32_t> d_kept;
    DevBuf<uint8_t> d_body;
    DevBuf<demod_frames_check_result_t> d_chk_sum;
    // the output block, device and pinned host: summary | states [S] | records
    // [S max_frames] | bytes [S max_frames max_len]. The states live here, so
    // they come back with the same copy.
    DevBuf<unsigned char> d_out;
    PinnedBuf<unsigned char> h_out;
    size_t out_bytes = 0;
    std::vector<uint32_t> counts;         // per push: each stream's new windows

    static constexpr size_t kStates = sizeof(demod_rx_summary_t);
    size_t frames_off() const { return kStates + S * sizeof(demod_rx_stream_state_t); }
    size_t bodies_off() const { return frames_off() + (size_t)sz.frames_bytes; }
    demod_rx_stream_state_t *d_state() { return reinterpret_cast<demod_rx_stream_state_t *>(d_out.p + kStates); }
    demod_rx_stream_state_t *h_state() const { return reinterpret_cast<demod_rx_stream_state_t *>(h_out.p + kStates); }
};

static int rx_allocate(demod_rx_t *rx)
{
    const demod_rx_sizes_t &z = rx->sz;
    const size_t S = rx->S, rows = S * rx->rx.max_frames;
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(rx->ring_sym[b].reserve(z.ring_sym_bytes));
        HIP_TRY(rx->ring_mag[b].reserve(z.ring_mag_bytes / sizeof(float)));
        HIP_TRY(hipMemset(rx->ring_sym[b].p, 0, z.ring_sym_bytes));
        HIP_TRY(hipMemset(rx->ring_mag[b].p, 0, z.ring_mag_bytes));
    }
    HIP_TRY(rx->d_first.reserve(S));
    HIP_TRY(rx->d_count.reserve(S));
    HIP_TRY(rx->d_scan_work.reserve(z.scan_work_bytes));
    if (rs_mode_conv(rs_erase_strip(rx->rx.fec))) {
        HIP_TRY(rx->d_fec_work.reserve(z.decode_work_bytes));
        HIP_TRY(rx->d_decode.reserve(rows));
    }
    if (rs_parity(rx->rx.fec)) HIP_TRY(rx->d_rs.reserve(rows));
    if (rs_erase_level(rx->rx.fec)) {
        HIP_TRY(rx->d_erase.reserve(rows * rs_mask_words((unsigned)z.row_bytes)));
        HIP_TRY(rx->d_erec.reserve(rows));
    }
    HIP_TRY(rx->d_col_work.reserve(z.collect_work_bytes));
    HIP_TRY(rx->d_hits.reserve(rows));
    HIP_TRY(rx->d_res.reserve(S));
    HIP_TRY(rx->d_rows.reserve(rows * z.row_bytes));
    HIP_TRY(rx->d_check.reserve(rows));
    HIP_TRY(rx->d_kept.reserve(rows));
    HIP_TRY(rx->d_body.reserve(rows * z.max_len + 1));
    HIP_TRY(rx->d_chk_sum.reserve(S));
    rx->out_bytes = rx->bodies_off() + (size_t)z.bodies_bytes;
    HIP_TRY(rx->d_out.reserve(rx->out_bytes + 1));
    HIP_TRY(rx->h_out.reserve(rx->out_bytes + 1));
    HIP_TRY(hipMemset(rx->d_out.p, 0, rx->frames_off()));
    std::memset(rx->h_out.p, 0, rx->frames_off());
    return DEMOD_OK;
}

extern "C" {

demod_rx_t *demod_rx_create(const demod_cfg_t *cfg, const demod_rx_cfg_t *rxcfg, size_t n_streams,
                            int *error)
{
    demod_rx_t *rx = nullptr;
    const auto done = [&](int code) {   // a failure leaves nothing behind
        if (code != DEMOD_OK) {
            demod_rx_destroy(rx);
            rx = nullptr;
        }
        if (error) *error = code;
        return rx;
    };
    demod_rx_sizes_t sz;
    int rc = demod_rx_sizes(cfg, rxcfg, n_streams, &sz);
    if (rc != DEMOD_OK) return done(rc);
    rx = new (std::nothrow) demod_rx();
    if (!rx) return done(DEMOD_ALLOC_FAIL);
    rx->cfg = *cfg;
    rx->rx = *rxcfg;
    rx->sz = sz;
    rx->S = n_streams;
    rx->ms = demod_streams_create(cfg, n_streams, &rc);
    if (!rx->ms) return done(rc);
    streams_copy_staging(rx->ms);
    try {
        rx->counts.assign(n_streams, 0);
    } catch (...) {
        return done(DEMOD_ALLOC_FAIL);
    }
    DeviceGuard guard(streams_device(rx->ms));
    if (guard.err != hipSuccess) return done(DEMOD_DEVICE_ERROR);
    return done(rx_allocate(rx));
}

void demod_rx_destroy(demod_rx_t *rx)
{
    if (!rx) return;
    demod_streams_destroy(rx->ms);
    delete rx;   // the buffers free themselves
}

int demod_rx_reset(demod_rx_t *rx, size_t stream)
{
    if (!rx || stream >= rx->S) return DEMOD_BAD_ARG;
    demod_t *st = streams_detector(rx->ms);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(hipMemsetAsync(rx->d_state() + stream, 0, sizeof(demod_rx_stream_state_t), st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    std::memset(rx->h_state() + stream, 0, sizeof(demod_rx_stream_state_t));
    return demod_streams_reset(rx->ms, stream);
}

int demod_rx_state(const demod_rx_t *rx, size_t stream, demod_rx_stream_state_t *state)
{
    if (!rx || !state || stream >= rx->S) return DEMOD_BAD_ARG;
    *state = rx->h_state()[stream];
    return DEMOD_OK;
}

// The device half of a push, on the detector handle's stream: the staged runs
// and the two tables behind them in, the stages, the output block out.
static int rx_run(demod_rx_t *rx, demod_t *st, const StreamsStage &sg)
{
    const demod_rx_cfg_t &x = rx->rx;
    const int level = (int)rs_erase_level(x.fec), fec = (int)rs_erase_strip(x.fec);   // the stages' mode
    const unsigned conv = rs_mode_conv((unsigned)fec);   // the trellis's mode, or 0: the scan writes packed rows
    const size_t S = rx->S, C = x.ring_windows, Wb = sg.Wb, mf = x.max_frames;
    const size_t L = x.sync_len, N = x.frame_symbols;
    // the tables of demod_segments_layout's layout, 16-byte aligned behind the samples
    const size_t t0 = (sg.samples + 7) / 8 * 8;
    uint64_t *h_first = reinterpret_cast<uint64_t *>(sg.base + t0);
    uint32_t *h_count = reinterpret_cast<uint32_t *>(h_first + S);
    for (size_t s = 0; s < S; ++s) {
        h_first[s] = sg.first[s];
        h_count[s] = rx->counts[s];
    }
    const size_t in_samples = t0 + 6 * S;
    int rc;
    if ((rc = ensure_dev(st, in_samples, Wb ? Wb : 1, true)) != DEMOD_OK) return rc;
    HIP_TRY(hipMemcpyAsync(st->d_in.p, sg.base, in_samples * sizeof(int16_t), hipMemcpyHostToDevice,
                           st->stream));
    if (Wb) {
        rc = enqueue_batch(st, st->d_in.p, Wb, st->d_sym.p, st->d_mag.p, st->stream);
        if (rc < 0) return rc;
    }
    const uint64_t *d_new_first = reinterpret_cast<const uint64_t *>(st->d_in.p + t0);
    const uint32_t *d_new_count = reinterpret_cast<const uint32_t *>(d_new_first + S);
    const int in = rx->cur, out = 1 - rx->cur;
    rc = demod_rx_advance_async(st, rx->d_state(), rx->ring_sym[in].p, rx->ring_mag[in].p, st->d_sym.p,
                                st->d_mag.p, Wb, d_new_first, d_new_count, S, C, rx->ring_sym[out].p,
                                rx->ring_mag[out].p, rx->d_first.p, rx->d_count.p, st->stream);
    if (rc < 0) return rc;
    rc = demod_frames_segments_async(st, rx->ring_sym[out].p, rx->ring_mag[out].p, S * C, rx->d_first.p,
                                     rx->d_count.p, S, x.sync, L, x.max_errors, N, rx->d_hits.p, nullptr,
                                     conv ? nullptr : rx->d_rows.p, mf, rx->d_res.p, rx->d_scan_work.p,
                                     rx->sz.scan_work_bytes, st->stream);
    if (rc < 0) return rc;
    uint8_t *d_body = rx->sz.max_len ? rx->d_body.p : nullptr;
    if (conv) {
        rc = demod_frames_decode_async(st, rx->d_hits.p, rx->ring_mag[out].p, S * C, rx->d_first.p, rx->d_res.p,
                                       S, mf, L, N, (int)x.len_bytes, (int)x.crc, fec, rx->d_rows.p,
                                       rx->d_decode.p, rx->d_fec_work.p, rx->sz.decode_work_bytes, st->stream);
        if (rc < 0) return rc;
    }
    if (level) {   // the packed rows' masks from the ring's powers, then the outer code with them
        rc = demod_frames_erasures_async(st, rx->d_hits.p, rx->ring_mag[out].p, S * C, rx->d_first.p, rx->d_res.p,
                                         S, mf, L, N, level, rx->d_erase.p, st->stream);
        if (rc < 0) return rc;
        rc = demod_frames_rs_erasures_async(st, rx->d_rows.p, rx->d_erase.p, rx->d_res.p, S, mf, N,
                                            (int)x.len_bytes, (int)x.crc, fec, rx->d_rs.p, rx->d_erec.p,
                                            st->stream);
        if (rc < 0) return rc;
    } else if (rs_parity((unsigned)fec)) {   // the outer code over the packed or the decoded rows, before the check
        rc = demod_frames_rs_async(st, rx->d_rows.p, rx->d_res.p, S, mf, N, (int)x.len_bytes, (int)x.crc,
                                   fec, rx->d_rs.p, st->stream);
        if (rc < 0) return rc;
    }
    if (fec) {
        rc = demod_frames_check_coded_async(st, rx->d_hits.p, rx->d_rows.p, rx->d_res.p, S, mf, L, N,
                                            (int)x.len_bytes, (int)x.crc, fec, rx->d_check.p,
                                            rx->d_kept.p, d_body, rx->d_chk_sum.p, st->stream);
    } else {
        rc = demod_frames_check_async(st, rx->d_hits.p, rx->d_rows.p, rx->d_res.p, S, mf, L, N,
                                      (int)x.len_bytes, (int)x.crc, rx->d_check.p, rx->d_kept.p, d_body,
                                      rx->d_chk_sum.p, st->stream);
    }
    if (rc < 0) return rc;
    rc = demod_rx_collect_async(st, rx->d_state(), rx->d_hits.p, rx->d_res.p, rx->d_check.p, rx->d_kept.p,
                                d_body, rx->d_chk_sum.p, S, mf, L, N, (int)x.len_bytes, (int)x.crc, fec,
                                reinterpret_cast<demod_rx_frame_t *>(rx->d_out.p + rx->frames_off()),
                                rx->d_out.p + rx->bodies_off(),
                                reinterpret_cast<demod_rx_summary_t *>(rx->d_out.p), rx->d_col_work.p,
                                rx->sz.collect_work_bytes, st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(rx->h_out.p, rx->d_out.p, rx->out_bytes, hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    return DEMOD_OK;
}

int demod_rx_push(demod_rx_t *rx, const int16_t *const *pcm, const size_t *n_frames,
                  const demod_rx_frame_t **frames, const uint8_t **bodies, demod_rx_summary_t *summary)
{
    if (!rx || !n_frames || !frames || !bodies || !summary) return DEMOD_BAD_ARG;
    demod_streams_t *ms = rx->ms;
    size_t Wb = 0;
    const long long Wc = streams_check(ms, pcm, n_frames, rx->counts.data(), streams_first(ms), &Wb);
    if (Wc < 0) return (int)Wc;
    demod_t *st = streams_detector(ms);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    StreamsStage sg;
    // behind the runs: up to 7 samples of padding, then 12 bytes of tables per stream
    int rc = streams_stage(ms, pcm, n_frames, (size_t)Wc, Wb, 8 + 6 * rx->S, &sg);
    if (rc != DEMOD_OK) return rc;
    rc = rx_run(rx, st, sg);
    if (rc < 0) {
        streams_unstage(ms, n_frames, sg);
        return rc;
    }
    streams_commit(ms, pcm, n_frames, rx->counts.data());
    rx->cur = 1 - rx->cur;
    *summary = *reinterpret_cast<const demod_rx_summary_t *>(rx->h_out.p);
    *frames = reinterpret_cast<const demod_rx_frame_t *>(rx->h_out.p + rx->frames_off());
    *bodies = rx->h_out.p + rx->bodies_off();
    return (int)summary->n_frames;
}

}  // extern "C"
