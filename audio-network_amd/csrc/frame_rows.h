/*
 * frame_rows.h — the row walk of the stages over a frame scan's rows (frames_check.hip, frames_fec.hip,
 * frames_rs.hip, frames_carry.hip, frames_tx.hip), once. Group (or stream) g of n_groups owns rows g max_frames
 * + i, i < nw_g = rows_clamped(the count stored in device memory, max_frames): every launch reads and clamps
 * the count itself, and that clamp is what keeps a poisoned count from indexing out of bounds. A launch gives
 * each group wpg waves of 64 lanes, four to a workgroup; wave c of a group takes rows c, c + wpg, .. below nw_g
 * (wave-uniform; a group without rows costs its waves one load). wpg is what the launch wants (a wave a row, or
 * one per 64 elements to move), held to kRowMaxWaves waves a call or one a group: include/demod.h's
 * min(max_frames, max(16384 / n_groups, 1)). The launch arithmetic is plain integer code that a C program
 * compiles too (tests/native); the rest is device code. Also here: what the frame scans share with the stages.
 */
#ifndef FSKD_FRAME_ROWS_H
#define FSKD_FRAME_ROWS_H

#ifdef __cplusplus
#include "demod_internal.h"
#include "frame_shape.h"
#define FRAME_ROWS_FN constexpr
namespace fskd {
#else
#define FRAME_ROWS_FN static inline
#endif

enum {
    kRowThreads = 256,                      /* a workgroup of the stages' launches */
    kRowLanes = 64,
    kRowWaves = kRowThreads / kRowLanes,
    kRowMaxWaves = 16384                    /* waves per call (or one per group) */
};

/* wpg of a launch over n_groups >= 1 groups that wants `want` waves a group */
FRAME_ROWS_FN unsigned row_waves_per_group(unsigned n_groups, unsigned long long want)
{
    const unsigned most = kRowMaxWaves / n_groups ? kRowMaxWaves / n_groups : 1u;
    return want < most ? (unsigned)want : most;
}

/* its workgroups: n_groups wpg <= max(kRowMaxWaves, n_groups) waves */
FRAME_ROWS_FN unsigned row_blocks(unsigned n_groups, unsigned wpg)
{
    return (unsigned)(((unsigned long long)n_groups * wpg + kRowWaves - 1) / kRowWaves);
}

#ifdef __HIPCC__

/* A wave's place in such a launch: wave gw of the call, first row c of group g; not live: no group, leave. */
struct RowWave {
    unsigned long long gw;
    unsigned g, c;
    bool live;
};

static __device__ __forceinline__ RowWave row_wave(unsigned n_groups, unsigned wpg)
{
    RowWave w;
    w.gw = (unsigned long long)blockIdx.x * kRowWaves + threadIdx.x / kRowLanes;
    const unsigned long long g = w.gw / wpg;
    w.live = g < n_groups;
    w.g = (unsigned)g;
    w.c = (unsigned)(w.gw % wpg);
    return w;
}

/* a count as a launch left it in device memory, held to the rows there are */
static __device__ __forceinline__ unsigned rows_clamped(unsigned long long stored, unsigned max_frames)
{
    return stored < max_frames ? (unsigned)stored : max_frames;
}

/* a row's length header of h = 1 or 2 bytes, highest first; the same in every lane of the wave */
static __device__ __forceinline__ unsigned row_length_load(const uint8_t *row, unsigned h)
{
    unsigned len = row[0];
    if (h == 2) len = (len << 8) | row[1];
    return (unsigned)__builtin_amdgcn_readfirstlane((int)len);
}

/* by lanes 0 .. h - 1 of the wave, a byte each */
static __device__ __forceinline__ void row_length_store(uint8_t *row, unsigned h, unsigned len, int lane)
{
    if ((unsigned)lane < h) row[lane] = (uint8_t)(len >> (8u * (h - 1u - (unsigned)lane)));
}

/* orders a wave's accesses to memory that no other wave touches (its own LDS slice) */
static __device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the frame scans: a hit at w is complete when w + frame_span is below the
// windows of its batch or segment, so that its word and payload fit. (The
// fields by reference, as the two units' own copies read them: by value the
// segmented scan kernel compiles to other machine code.)
__device__ __forceinline__ long long frame_span(const int &sync_len, const long long &frame_symbols,
                                                const int &phases)
{
    return ((long long)sync_len + frame_symbols - 1) * phases;
}

// byte b of a frame's packed row; src: the payload's first symbol, the next R
// bytes on. MSB first, each symbol masked to `bits` bits (mask: the caller's
// (1 << bits) - 1), pad bits 0 (demod_pack_symbols). One thread per byte, so no
// two threads share one.
__device__ __forceinline__ uint8_t frame_packed_byte(const uint8_t *src, unsigned long long R,
                                                     unsigned long long N, unsigned bits, unsigned mask,
                                                     unsigned long long b)
{
    unsigned q = 0;   // bits of the byte filled
    unsigned long long j = b * 8 / bits;
    unsigned used = (unsigned)(b * 8 - j * bits);   // bits of symbol j in the bytes before
    unsigned byte = 0;
    while (q < 8 && j < N) {
        const unsigned v = src[j * R] & mask;
        const unsigned left = bits - used, room = 8 - q;
        const unsigned take = left < room ? left : room;
        byte |= ((v >> (left - take)) & ((1u << take) - 1u)) << (room - take);
        q += take;
        used += take;
        if (used == bits) {
            used = 0;
            ++j;
        }
    }
    return (uint8_t)byte;
}

// the symbols a checked frame of `length` data bytes occupies behind its word: frame_shape.h's span, coded
// where the check runs over decoded rows (fec_depth). `covered` (frames_check.hip), `hold` (frames_carry.hip).
__device__ __forceinline__ unsigned checked_frame_span(unsigned length, unsigned len_bytes, unsigned crc_bytes,
                                                       unsigned bits, unsigned fec_depth, unsigned fec,
                                                       unsigned parity)
{
    unsigned T, Nt;
    return frame_air_symbols(length, len_bytes, crc_bytes, bits, fec_depth ? fec : 0u, parity, &T, &Nt);
}

#endif  /* __HIPCC__ */

#ifdef __cplusplus
}  // namespace fskd
#endif

#endif
