// demod_frames.cpp — the C ABI of the stages over a frame scan's rows (include/demod.h "checked frames", "coded
// frames", "Reed-Solomon outer code"): the check (frames_check.hip), the Viterbi decode (frames_fec.hip) and the
// outer code (frames_rs.hip), each an *_async call on device memory and the caller's stream, and the one-shot
// calls that run detector, scan and stages on the handle's stream. The row's shape is frame_shape.h's; the
// scans themselves are demod_acquire.cpp's.
#include <cstring>

#include "demod_host.h"
#include "frame_rows.h"

using namespace fskd;

// The check's launch. fec 0: the scan's packed rows; else decoded rows (the coded entry has refused fec 0).
static int frames_check_enqueue(demod_t *st, const demod_frame_hit_t *d_hits, const uint8_t *d_packed,
                                const demod_frames_result_t *d_results, size_t n_groups,
                                size_t max_frames, size_t sync_len, size_t frame_symbols, int len_bytes,
                                int crc, int fec, demod_frame_check_t *d_check, uint32_t *d_kept,
                                uint8_t *d_body, demod_frames_check_result_t *d_summary, void *stream)
{
    if (!st || !d_hits || !d_packed || !d_results || !d_check || !d_kept || !d_summary) return DEMOD_BAD_ARG;
    if (!aligned8(d_hits, d_results, d_summary) || !aligned4(d_check, d_kept)) return DEMOD_BAD_ARG;
    frame_shape s;
    const uint32_t R = stage_shape(st->cfg, n_groups, max_frames, sync_len, frame_symbols, len_bytes, crc, fec, s);
    if (R == 0) return DEMOD_BAD_ARG;
    FramesCheckParams p;
    std::memset(&p, 0, sizeof(p));
    fill_shape_fields(p, s, max_frames, R, sync_len);
    fill_crc_fields(p, s.crc_bytes);
    p.n_groups = (unsigned)n_groups;
    p.row_bytes = s.row_bytes;
    p.fec_depth = s.fec_depth;
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

// demod_frames_checked (fec 0: the scan's packed rows) and demod_frames_coded
static int frames_checked_run(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                              size_t sync_len, uint32_t max_errors, size_t frame_symbols, int len_bytes,
                              int crc, int fec, demod_frame_hit_t *hits, uint32_t *lengths, uint8_t *body,
                              size_t max_frames, demod_frames_result_t *result,
                              demod_frames_check_result_t *summary)
{
    if (!st || !pcm || !result || !summary || !hits || !lengths || ((uintptr_t)pcm & 15) != 0)
        return DEMOD_BAD_ARG;
    const uint32_t R = frames_args(st->cfg, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames, true);
    if (R == 0) return DEMOD_BAD_ARG;   // before the detector runs
    const size_t dcap = hit_cap(max_frames, n_windows, R);
    const int level = (int)rs_erase_level((unsigned)fec);   // of "erasure decoding": this call's own
    fec = (int)rs_erase_strip((unsigned)fec);               // the stages' mode
    frame_shape s;
    if (!stage_shape(st->cfg, 1, dcap, sync_len, frame_symbols, len_bytes, crc, fec, s)) return DEMOD_BAD_ARG;
    unsigned mask_row = 0;   // with a level: what the producer will ask, before anything is queued
    if (level && (!erasures_shape(st->cfg, 1, dcap, sync_len, frame_symbols, mask_row) || mask_row != s.row_bytes))
        return DEMOD_BAD_ARG;
    const int conv = s.fec;   // the trellis's mode or 0 (the scan's packed rows); s.parity: the outer code's stage
    const size_t fec_work = conv ? demod_fec_decode_workspace_size(&st->cfg, 1, dcap, frame_symbols, conv) : 0;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    const size_t N = frame_symbols, B = s.row_bytes, M = s.max_len;
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
    if (s.parity) HIP_TRY(st->d_rs.reserve(dcap));
    if (level) {
        HIP_TRY(st->d_erase.reserve(dcap * rs_mask_words(s.row_bytes)));
        HIP_TRY(st->d_erec.reserve(dcap));
    }
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
    if (level) {   // the packed rows' masks from the powers, then the outer code with them
        rc = demod_frames_erasures_async(st, st->d_frm_hits.p, st->d_mag.p, n_windows, nullptr, st->d_frm_res.p, 1,
                                         dcap, sync_len, N, level, st->d_erase.p, st->stream);
        if (rc < 0) return rc;
        rc = demod_frames_rs_erasures_async(st, rows, st->d_erase.p, st->d_frm_res.p, 1, dcap, N, len_bytes, crc,
                                            fec, st->d_rs.p, st->d_erec.p, st->stream);
        if (rc < 0) return rc;
    } else if (s.parity) {
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

// The outer code's stage, with or without masks: its refusals and the launch's fields.
static int frames_rs_params(demod_t *st, uint8_t *d_rows, const demod_frames_result_t *d_results, size_t n_groups,
                            size_t max_frames, size_t frame_symbols, int len_bytes, int crc, int fec,
                            demod_frame_rs_t *d_rs, FramesRsParams &p)
{
    if (!st || !d_rows || !d_results || !d_rs) return DEMOD_BAD_ARG;
    if (((uintptr_t)d_results & 7) != 0 || ((uintptr_t)d_rs & 3) != 0) return DEMOD_BAD_ARG;
    if (!rs_mode_valid((unsigned)fec) || !rs_parity((unsigned)fec)) return DEMOD_BAD_ARG;
    frame_shape s;   // the shape the coded check will see: the same refusals (it has no word here)
    if (!stage_shape(st->cfg, n_groups, max_frames, 1, frame_symbols, len_bytes, crc, fec, s)) return DEMOD_BAD_ARG;
    std::memset(&p, 0, sizeof(FramesRsParams));
    p.n_groups = (unsigned)n_groups;
    p.max_frames = (unsigned)max_frames;
    p.row_bytes = s.row_bytes;
    p.max_len = s.max_len;
    p.len_bytes = s.len_bytes;
    p.crc_bytes = s.crc_bytes;
    p.parity = s.parity;
    p.rows = d_rows;
    p.res = d_results;
    p.rs = d_rs;
    return DEMOD_OK;
}

extern "C" {

// ---- checked frames (frames_check.hip) ---------------------------------------

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
    const unsigned conv = rs_mode_conv((unsigned)fec);   // a parity flag does not change the trellis's workspace
    if (validate_cfg(cfg) != DEMOD_OK || cfg->k < 2 || (cfg->k & (cfg->k - 1)) != 0) return 0;
    if (!group_rows_ok(n_groups, max_frames, false) || frame_symbols == 0 || frame_symbols > 0x7FFFFFFF) return 0;
    const size_t St = frame_row_steps(conv, frame_symbols * (size_t)demod_bits_per_symbol(cfg->k));
    return n_groups * (size_t)row_waves_per_group((unsigned)n_groups, (unsigned)max_frames) * St * 8;
}

int demod_frames_decode_async(demod_t *st, const demod_frame_hit_t *d_hits, const float *d_mags,
                              size_t n_windows, const uint64_t *d_first,
                              const demod_frames_result_t *d_results, size_t n_groups,
                              size_t max_frames, size_t sync_len, size_t frame_symbols, int len_bytes,
                              int crc, int fec, uint8_t *d_rows, demod_frame_decode_t *d_decode,
                              void *d_work, size_t work_bytes, void *stream)
{
    if (!st || !d_hits || !d_mags || !d_results || !d_rows || !d_decode || !d_work) return DEMOD_BAD_ARG;
    if (!aligned8(d_hits, d_results, d_work, d_first) || !aligned4(d_decode)) return DEMOD_BAD_ARG;
    if (!rs_mode_valid((unsigned)fec) || !rs_mode_conv((unsigned)fec) || n_windows > 0x7FFFFFFF)
        return DEMOD_BAD_ARG;
    frame_shape s;   // the shape the coded check will see: the same refusals
    const uint32_t R = stage_shape(st->cfg, n_groups, max_frames, sync_len, frame_symbols, len_bytes, crc, fec, s);
    if (R == 0 || (sync_len + frame_symbols) * (size_t)R > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    const size_t need = demod_fec_decode_workspace_size(&st->cfg, n_groups, max_frames, frame_symbols, s.fec);
    if (need == 0 || work_bytes < need) return DEMOD_BAD_ARG;
    FramesFecParams p;
    std::memset(&p, 0, sizeof(p));
    fill_shape_fields(p, s, max_frames, R, sync_len);
    p.n_groups = (unsigned)n_groups;
    p.row_bytes = s.row_bytes;
    p.steps = s.steps;
    p.hits = d_hits;
    p.mag = d_mags;
    p.first = reinterpret_cast<const unsigned long long *>(d_first);
    p.res = d_results;
    p.n_windows = (unsigned)n_windows;
    p.frame_symbols = (unsigned)frame_symbols;
    p.k = (int)st->cfg.k;
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

// ---- Reed-Solomon outer code (frames_rs.hip) -----------------------------------

int demod_frames_rs_async(demod_t *st, uint8_t *d_rows, const demod_frames_result_t *d_results,
                          size_t n_groups, size_t max_frames, size_t frame_symbols, int len_bytes, int crc,
                          int fec, demod_frame_rs_t *d_rs, void *stream)
{
    FramesRsParams p;
    const int rc = frames_rs_params(st, d_rows, d_results, n_groups, max_frames, frame_symbols, len_bytes, crc, fec,
                                    d_rs, p);
    if (rc != DEMOD_OK) return rc;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_frames_rs(p, (hipStream_t)stream));
    return DEMOD_OK;
}

// ---- erasure decoding (frames_erasures.hip, frames_rs.hip) ------------------------

int demod_frames_erasures_async(demod_t *st, const demod_frame_hit_t *d_hits, const float *d_mags,
                                size_t n_windows, const uint64_t *d_first,
                                const demod_frames_result_t *d_results, size_t n_groups, size_t max_frames,
                                size_t sync_len, size_t frame_symbols, int level, uint64_t *d_erase,
                                void *stream)
{
    if (!st || !d_hits || !d_mags || !d_results || !d_erase) return DEMOD_BAD_ARG;
    if (!aligned8(d_hits, d_results, d_first, d_erase) || !aligned4(d_mags)) return DEMOD_BAD_ARG;
    if (level < 1 || level > 127 || n_windows > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    unsigned B;   // plain rows: the packed row's width is all of a row's shape that is used
    const uint32_t R = erasures_shape(st->cfg, n_groups, max_frames, sync_len, frame_symbols, B);
    if (R == 0) return DEMOD_BAD_ARG;
    FramesEraseParams p;
    std::memset(&p, 0, sizeof(p));
    p.hits = d_hits;
    p.mag = d_mags;
    p.first = reinterpret_cast<const unsigned long long *>(d_first);
    p.res = d_results;
    p.n_windows = (unsigned)n_windows;
    p.n_groups = (unsigned)n_groups;
    p.max_frames = (unsigned)max_frames;
    p.frame_symbols = (unsigned)frame_symbols;
    p.row_bytes = B;
    p.k = (int)st->cfg.k;
    p.bits = demod_bits_per_symbol(st->cfg.k);
    p.phases = (int)R;
    p.sync_len = (int)sync_len;
    p.level = level;
    p.erase = d_erase;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_frames_erasures(p, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_frames_rs_erasures_async(demod_t *st, uint8_t *d_rows, const uint64_t *d_erase,
                                   const demod_frames_result_t *d_results, size_t n_groups, size_t max_frames,
                                   size_t frame_symbols, int len_bytes, int crc, int fec,
                                   demod_frame_rs_t *d_rs, demod_frame_erase_t *d_erec, void *stream)
{
    FramesRsEraseParams p;
    if (!d_erase || !d_erec || !aligned8(d_erase) || !aligned4(d_erec)) return DEMOD_BAD_ARG;
    const int rc = frames_rs_params(st, d_rows, d_results, n_groups, max_frames, frame_symbols, len_bytes, crc, fec,
                                    d_rs, p);
    if (rc != DEMOD_OK) return rc;
    p.erase = d_erase;
    p.erec = d_erec;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_frames_rs_erasures(p, (hipStream_t)stream));
    return DEMOD_OK;
}

// ---- the one-shot calls ----------------------------------------------------------

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
    if (!rs_erase_mode_valid((unsigned)fec)) return DEMOD_BAD_ARG;   // alone here: with or without a level
    return frames_checked_run(st, pcm, n_windows, sync, sync_len, max_errors, frame_symbols, len_bytes, crc,
                              fec, hits, lengths, body, max_frames, result, summary);
}

}  // extern "C"
