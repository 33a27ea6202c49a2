// stream_stage.h — how demod_streams_push lays many streams out as one batch
// (host only: no HIP). A push puts the streams' runs of complete windows end
// to end, each run starting on a multiple of hop, so the batch is an ordinary
// hop-strided window sequence: stream s's windows are batch windows
// first[s] .. first[s] + W_s - 1, and the ceil(L_s / hop) - W_s windows that
// start inside its run but end past it (n / hop - 1 of them when hop divides
// n; none at hop = n) straddle into the next run and are computed and
// dropped. demod_streams.cpp runs these on its staging threads;
// tests/native/stream_stage_test.cpp against a naive model under ASan + UBSan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/demod.h"

namespace fskd {

// The mono samples of n_frames frames (cfg.channels interleaved): the
// channel cfg.channel_mode selects, or (L + R) >> 1.
inline void mono_frames(const demod_cfg_t &c, const int16_t *pcm, size_t n_frames, int16_t *dst)
{
    if (c.channels == 1) {
        if (n_frames) std::memcpy(dst, pcm, n_frames * sizeof(int16_t));
    } else if (c.channel_mode == DEMOD_CH_DOWNMIX) {
        for (size_t i = 0; i < n_frames; ++i)
            dst[i] = (int16_t)(((int32_t)pcm[2 * i] + (int32_t)pcm[2 * i + 1]) >> 1);
    } else {
        const int ch = c.channel_mode == DEMOD_CH_RIGHT ? 1 : 0;
        for (size_t i = 0; i < n_frames; ++i) dst[i] = pcm[2 * i + ch];
    }
}

// Complete windows of length n at stride hop in `total` samples.
inline size_t windows_for(size_t total, size_t n, size_t hop)
{
    return total < n ? 0 : (total - n) / hop + 1;
}

// The batch layout of S streams, stream s holding total(s) samples (carry +
// fresh frames): first[s] = the batch window of its first (nullable), counts[s]
// = its windows (nullable), *W = their sum. Returns Wb, the batch's windows:
// a run of w windows is L = (w - 1) hop + n samples and takes ceil(L / hop)
// batch slots.
template <class Total>
inline size_t run_layout(size_t S, size_t n, size_t hop, Total total, size_t *first,
                         uint32_t *counts, size_t *W)
{
    size_t sum = 0, Wb = 0;
    for (size_t s = 0; s < S; ++s) {
        const size_t w = windows_for(total(s), n, hop);
        if (first) first[s] = Wb;
        if (counts) counts[s] = (uint32_t)w;
        sum += w;
        if (w) Wb += ((w - 1) * hop + n + hop - 1) / hop;
    }
    *W = sum;
    return Wb;
}

// One stream of a push: its carry (hv samples in carry[], capacity >= n - 1)
// followed by the mono view of its f fresh frames (src, cfg.channels
// interleaved) goes to its run b, one host copy of the packet, written only
// within the run's own ceil(L / hop) hops, so streams are independent. The
// new carry (the samples past its last window's start + hop, < n) is formed
// in carry[] from the old carry and the packet. Returns the new carry length;
// a stream without a complete window is left alone (returns hv).
inline size_t stage_stream(const demod_cfg_t &c, const int16_t *src, size_t f, int16_t *carry,
                           size_t hv, int16_t *b)
{
    const size_t n = c.n, hop = c.hop, total = hv + f, w = windows_for(total, n, hop);
    if (!w) return hv;
    const size_t L = (w - 1) * hop + n, span = (L + hop - 1) / hop * hop;
    const size_t end = std::min(total, span);  // hv < n <= L <= end
    if (hv) std::memcpy(b, carry, hv * sizeof(int16_t));
    mono_frames(c, src, end - hv, b + hv);
    // the straddling windows read up to the next run's start: keep the gap
    // defined (their results are dropped)
    if (span > L) std::memset(b + L, 0, (span - L) * sizeof(int16_t));
    const size_t t0 = w * hop;  // new carry = samples [t0, total) of the stream
    if (t0 >= hv) {
        mono_frames(c, src + (t0 - hv) * c.channels, total - t0, carry);
    } else {
        std::memmove(carry, carry + t0, (hv - t0) * sizeof(int16_t));
        mono_frames(c, src, f, carry + (hv - t0));
    }
    return total - t0;
}

// The rollback of stage_stream when the batch fails (nothing consumed): the
// old carry is the run's first hv samples (hv < n <= L, below the run's gap
// fill; no other run writes there). Returns the restored carry length.
inline size_t unstage_stream(const demod_cfg_t &c, size_t f, int16_t *carry, size_t hv,
                             const int16_t *b)
{
    if (hv && windows_for(hv + f, c.n, c.hop)) std::memcpy(carry, b, hv * sizeof(int16_t));
    return hv;
}

}  // namespace fskd
