// frames_fec.hip — coded frames (include/demod.h "coded frames", DESIGN.md §4.9
// "Coded frames"): the soft values of the rows a frame scan listed, from the
// detector's per-tone powers, and their soft-decision Viterbi decode under the
// constraint-length-7, rate-1/2 code 0171/0133, in order or punctured to 2/3 or
// 3/4 and interleaved (fec_map.h: the trellis does not change, a soft value's
// place on the air does). The 64 trellis states are one wave: lane = state.
// Groups, rows and the walk as frame_rows.h, one wave per row. One launch, no
// atomics; every output byte is a function of the inputs alone
// (demod_fec.c's demod_coded_frame_decode restates it on the host).
//
//  soft     64 values at a time, one per lane: trellis value m sits at air
//           position a(m) (a = m without a map; a punctured m is 0 and reads
//           nothing); air value a = j bits + b of the row
//           reads the K powers of window base + window + (L + j) R and keeps
//           the largest with bit b clear and with bit b set. A window at or
//           past n_windows is an erasure (0) and is not read.
//  forward  lane s holds M[s]. Its predecessors are p0 = s >> 1 and p1 = p0 |
//           32, read by two ds_bpermute. The branch from p0 has register s, the
//           one from p1 register s | 64; both generators have bit 6 set, so the
//           second branch metric is minus the first, and the first's two signs
//           are lane constants. __ballot of the decision is the step's survivor
//           word. A pass of up to 32 steps keeps step i's word in lane i and
//           stores the words with one coalesced store to the wave's slot of
//           d_work ([waves of the launch][St] words).
//  header   at t0 = 8 h + DEMOD_FEC_DEPTH: the best state (the wave's maximum,
//           then the lowest lane that holds it), traced back to step 0.
//  trace    serial in the state: 64 words per load (lane i holds step 64 c +
//           i's), then one lane read and a shift per step on wave-uniform
//           values. The 64 input bits of a chunk are 8 row bytes, stored by
//           lanes 0 .. 7 where they are below the bytes to write.
//
// The forward pass stops at t0 for the header and at T(len) for the row: the
// outputs do not depend on later steps. A wave's loads of its slot follow its
// own stores in program order behind a workgroup fence.
#include "frame_rows.h"
#include "soft_ops.h"

namespace fskd {

constexpr unsigned kFecPass = kRowLanes / 2;   // steps of one pass: 64 soft values

// trellis soft value m of a row whose symbol 0 of the word sits at window bw.
// MAPPED (fec_map.h): m is kept or not, then its code index, then its air
// position a < Cu <= N bits; a punctured m is 0 and loads nothing. Not MAPPED
// (DEMOD_FEC_CONV_K7 alone): a = m, and the code is what it was without a map.
template <bool MAPPED>
static __device__ __forceinline__ int fec_soft(const FramesFecParams &p, bool live,
                                               unsigned long long bw, unsigned m)
{
    if (!live || m >= 2u * p.steps) return 0;
    if (MAPPED) {
        m = fec_air_of_mother(p.fec, m);
        if (m == FEC_MAP_NONE) return 0;
    }
    return soft_air_value(p.mag, p.n_windows, (unsigned)p.k, (unsigned)p.bits, (unsigned)p.sync_len,
                          (unsigned)p.phases, bw, m);   // m / bits < N
}

struct FecLane {
    int sgn0, sgn1;   // the branch from p0: -1 where the expected bit is 1
    int at0, at1;     // ds_bpermute addresses of p0 and p1
};

// steps t .. t + count - 1, count <= kFecPass and t + count <= St
template <bool MAPPED>
static __device__ __forceinline__ void fec_steps(const FramesFecParams &p, const FecLane &c, bool live,
                                                 unsigned long long bw, unsigned t, unsigned count,
                                                 int &M, unsigned long long *slot, int lane)
{
    const int q = fec_soft<MAPPED>(p, live && (unsigned)lane < 2u * count, bw, 2u * t + (unsigned)lane);
    unsigned long long mine = 0;
#pragma unroll 4
    for (unsigned i = 0; i < count; ++i) {
        const int q0 = __builtin_amdgcn_readlane(q, (int)(2u * i));
        const int q1 = __builtin_amdgcn_readlane(q, (int)(2u * i + 1u));
        const int bm = c.sgn0 * q0 + c.sgn1 * q1;
        const int a = __builtin_amdgcn_ds_bpermute(c.at0, M) + bm;
        const int b = __builtin_amdgcn_ds_bpermute(c.at1, M) - bm;
        const bool d = b > a;
        M = d ? b : a;
        const unsigned long long word = __ballot(d);
        if ((unsigned)lane == i) mine = word;
    }
    if ((unsigned)lane < count) slot[t + (unsigned)lane] = mine;
}

// u_t of steps t_end - 1 .. 0 from state s at step t_end (t_end >= 1). Row bytes
// below n_write are stored where row is given. Returns u_0 .. u_63, u_0 highest.
static __device__ __forceinline__ unsigned long long fec_trace(const unsigned long long *slot,
                                                               unsigned t_end, unsigned s, uint8_t *row,
                                                               unsigned n_write, int lane)
{
    s = (unsigned)__builtin_amdgcn_readfirstlane((int)s);
    unsigned long long acc = 0;
    for (int ch = (int)((t_end - 1u) / 64u); ch >= 0; --ch) {
        const unsigned tb = (unsigned)ch * 64u;
        const unsigned cnt = t_end - tb < 64u ? t_end - tb : 64u;
        const unsigned long long w = (unsigned)lane < cnt ? slot[tb + (unsigned)lane] : 0ull;
        const int lo = (int)(unsigned)w, hi = (int)(unsigned)(w >> 32);
        acc = 0;
        for (int i = (int)cnt - 1; i >= 0; --i) {
            acc |= (unsigned long long)(s & 1u) << (63 - i);
            const unsigned half = (unsigned)__builtin_amdgcn_readlane(s & 32u ? hi : lo, i);
            s = (s >> 1) | (((half >> (s & 31u)) & 1u) << 5);
        }
        const unsigned at = tb / 8u + (unsigned)lane;
        if (row && lane < 8 && at < n_write) row[at] = (uint8_t)(acc >> (56 - 8 * lane));
    }
    return acc;
}

template <bool MAPPED>
__global__ __launch_bounds__(kRowThreads) void frames_decode_kernel(FramesFecParams p, unsigned wpg)
{
    const int lane = threadIdx.x % kRowLanes;
    const RowWave rw = row_wave(p.n_groups, wpg);
    if (!rw.live) return;
    const unsigned g = rw.g;
    const unsigned nw = rows_clamped(p.res[g].n_written, p.max_frames);
    unsigned long long base = 0;
    if (p.first) base = p.first[g] < p.n_windows ? p.first[g] : p.n_windows;
    unsigned long long *slot = p.work + (size_t)rw.gw * p.steps;   // gw < n_groups wpg
    FecLane c;
    c.sgn0 = (__popc((unsigned)lane & 0171u) & 1) ? -1 : 1;
    c.sgn1 = (__popc((unsigned)lane & 0133u) & 1) ? -1 : 1;
    c.at0 = (lane >> 1) * 4;
    c.at1 = ((lane >> 1) | 32) * 4;
    const unsigned h = (unsigned)p.len_bytes, t0 = 8u * h + DEMOD_FEC_DEPTH;   // t0 <= St
    for (unsigned i = rw.c; i < nw; i += wpg) {   // the same for every lane of the wave
        const size_t r = (size_t)g * p.max_frames + i;
        const unsigned long long window = p.hits[r].window;
        const bool live = window < p.n_windows;   // else every value an erasure; no wrap below
        const unsigned long long bw = live ? base + window : 0;
        int M = lane == 0 ? 0 : -(1 << 28);
        for (unsigned t = 0; t < t0; t += kFecPass)
            fec_steps<MAPPED>(p, c, live, bw, t, t0 - t < kFecPass ? t0 - t : kFecPass, M, slot, lane);
        __threadfence_block();
        int mx = M;
        for (int d = kRowLanes / 2; d > 0; d >>= 1) {
            const int y = __shfl_xor(mx, d);
            if (y > mx) mx = y;
        }
        const unsigned best = (unsigned)__ffsll((long long)__ballot(M == mx)) - 1u;
        const unsigned long long head = fec_trace(slot, t0, best, nullptr, 0, lane);
        const unsigned len = (unsigned)(head >> (64u - 8u * h));
        uint8_t *row = p.rows + r * p.row_bytes;
        demod_frame_decode_t out;
        out.length = len;
        if (len > p.max_len) {
            row_length_store(row, h, len, lane);
            out.metric = 0;
            out.status = DEMOD_DECODE_BAD_LENGTH;
            out.steps = 0;
        } else {
            // the row's bytes: n, or n' with an outer code (rs_ops.h); <= row_bytes
            const unsigned n = rs_frame_bytes(h + len + (unsigned)p.crc_bytes, p.parity);
            const unsigned T = 8u * n + 6u > t0 ? 8u * n + 6u : t0;         // <= St
            for (unsigned t = t0; t < T; t += kFecPass)
                fec_steps<MAPPED>(p, c, live, bw, t, T - t < kFecPass ? T - t : kFecPass, M, slot, lane);
            __threadfence_block();
            fec_trace(slot, T, 0u, row, n, lane);
            out.metric = __builtin_amdgcn_readfirstlane(M);   // lane 0: state 0
            out.status = DEMOD_DECODE_OK;
            out.steps = T;
        }
        if (lane == 0) p.decode[r] = out;
    }
}

hipError_t launch_frames_decode(const FramesFecParams &p, hipStream_t s)
{
    const unsigned wpg = row_waves_per_group(p.n_groups, p.max_frames), blocks = row_blocks(p.n_groups, wpg);
    if (fec_mode_mapped(p.fec))
        hipLaunchKernelGGL(frames_decode_kernel<true>, dim3(blocks), dim3(kRowThreads), 0, s, p, wpg);
    else
        hipLaunchKernelGGL(frames_decode_kernel<false>, dim3(blocks), dim3(kRowThreads), 0, s, p, wpg);
    return hipGetLastError();
}

}  // namespace fskd
