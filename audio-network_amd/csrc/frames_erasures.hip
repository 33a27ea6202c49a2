// frames_erasures.hip — the erasure mask's producer (include/demod.h "erasure
// decoding", DESIGN.md §4.9 "Erasure decoding"): which bytes of the plain rows
// a frame scan listed the detector's powers call doubtful. Byte b of a row is
// flagged when the least |q_m| over its eight air bits m = 8 b .. 8 b + 7 is
// below the level; q_m is soft_ops.h's value at air position m, 0 for m >= N
// bits or a window at or past n_windows (neither is read). Groups, rows and the
// walk as frame_rows.h: a wave takes 64 consecutive bytes of a row, a thread a
// byte; the wave's ballot is one word of the mask, stored by lane 0. Every
// word of every row below the clamped count is written, no other. One launch,
// no workspace, no atomics; every word is a function of the inputs alone
// (demod_soft_bits and demod_soft_erasures restate it on the host).
#include "frame_rows.h"
#include "soft_ops.h"

namespace fskd {

__global__ __launch_bounds__(kRowThreads) void frames_erasures_kernel(FramesEraseParams p, unsigned wpg)
{
    const unsigned lane = threadIdx.x % kRowLanes;
    const RowWave rw = row_wave(p.n_groups, wpg);
    if (!rw.live) return;
    const unsigned g = rw.g;
    const unsigned nw = rows_clamped(p.res[g].n_written, p.max_frames);
    unsigned long long base = 0;
    if (p.first) base = p.first[g] < p.n_windows ? p.first[g] : p.n_windows;
    const unsigned Wm = rs_mask_words(p.row_bytes);
    const unsigned long long units = (unsigned long long)nw * Wm;   // the words of the group's rows
    const unsigned air = p.frame_symbols * (unsigned)p.bits;         // N bits <= 8 row_bytes, which the host held to a frame's
    for (unsigned long long u = rw.c; u < units; u += wpg) {   // the same for every lane of the wave
        const unsigned i = (unsigned)(u / Wm), wd = (unsigned)(u % Wm);   // i < nw <= max_frames
        const size_t r = (size_t)g * p.max_frames + i;
        const unsigned long long window = p.hits[r].window;
        const bool live = window < p.n_windows;   // else every value 0; no wrap below
        const unsigned long long bw = live ? base + window : 0;
        const unsigned b = wd * kRowLanes + lane;
        bool flag = false;
        if (b < p.row_bytes) {
            int least = 128;
            for (unsigned m = 8u * b; m < 8u * b + 8u; ++m) {
                int q = 0;
                if (live && m < air)
                    q = soft_air_value(p.mag, p.n_windows, (unsigned)p.k, (unsigned)p.bits, (unsigned)p.sync_len,
                                       (unsigned)p.phases, bw, m);
                q = q < 0 ? -q : q;
                if (q < least) least = q;
            }
            flag = least < p.level;
        }
        const unsigned long long word = __ballot(flag);
        if (lane == 0) p.erase[r * Wm + wd] = word;
    }
}

hipError_t launch_frames_erasures(const FramesEraseParams &p, hipStream_t s)
{
    const unsigned long long want = (unsigned long long)p.max_frames * rs_mask_words(p.row_bytes);
    const unsigned wpg = row_waves_per_group(p.n_groups, want), blocks = row_blocks(p.n_groups, wpg);
    hipLaunchKernelGGL(frames_erasures_kernel, dim3(blocks), dim3(kRowThreads), 0, s, p, wpg);
    return hipGetLastError();
}

}  // namespace fskd
