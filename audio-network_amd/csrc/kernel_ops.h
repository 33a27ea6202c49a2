// kernel_ops.h — device helpers the detector kernels share on top of the
// host/kernel contract (demod_internal.h): the two-stage ambiguity test, the
// K-tone chain decision, a lane segment's fp32 energy, the XCD tile swizzle
// and the write-back bursts. Device only: no host translation unit includes
// this.
#pragma once
#include "demod_internal.h"
#include "lane_ops.h"
#include "rescue_ops.h"

namespace fskd {

// stage 1: margin within tau sqrt(Q P_max) (amb_tq = tau sqrt(Q)), or
// P_max == 0 (a candidate: stage 2 asks for energy)
__device__ __forceinline__ bool amb_margin(float p1, float p2, float tq, float fl)
{
    return tq > 0.f && (p1 == 0.f || p1 - p2 < tq * __builtin_amdgcn_sqrtf(p1) || p1 < fl);
}

// stage 2: (p1 - p2)^2 < t2e E p1, or p1 below the floor t2e E / 16, or p1 ==
// 0 with E > 0
__device__ __forceinline__ bool amb_energy(float p1, float p2, float e, float t2e)
{
    const float c = t2e * e, d = p1 - p2;
    return p1 > 0.f ? (d * d < c * p1 || 16.f * p1 < c) : c > 0.f;
}

// The two stages over a wave: `amb1` is this lane's stage-1 verdict (false for
// lanes without a real window); efn() returns the lane's row energy E and is
// called by every lane (it may shuffle), only when some lane of the wave has
// amb1 set (a wave-uniform branch: nothing is spent on unflagged waves).
template <typename EFn>
__device__ __forceinline__ bool amb_two_stage(bool amb1, float p1, float p2, float t2e, EFn efn)
{
    if (__ballot(amb1) == 0) return false;
    const float e = efn();
    return amb1 && amb_energy(p1, p2, e, t2e);
}

// Sequential argmax (ties to the lowest k) that also keeps the runner-up, for
// the detectors' K-tone chains where every lane holds every P_k.
template <int K>
__device__ __forceinline__ int chain_argmax(const float (&P)[K], float &p1, float &p2)
{
    float best = -1.f, second = -1.f;
    int arg = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (P[k] > best) {
            second = best;
            best = P[k];
            arg = k;
        } else if (P[k] > second) {
            second = P[k];
        }
    }
    p1 = best;
    p2 = second;
    return arg;
}

// A chain decision (K >= 2 flags ambiguous windows): the argmax, and the
// two-stage ambiguity verdict (stage 2 via efn, see amb_two_stage; `live` =
// the lane's window exists).
template <int K, typename EFn>
__device__ __forceinline__ int chain_decide(const float (&P)[K], bool live, float tq, float fl, float t2e,
                                            EFn efn, bool &amb)
{
    float p1, p2;
    const int arg = chain_argmax<K>(P, p1, p2);
    amb = K >= 2 && amb_two_stage(live && amb_margin(p1, p2, tq, fl), p1, p2, t2e, efn);
    return arg;
}

// Sum of squares of the 64 int16 samples of one lane segment, 16-byte chunks
// read by `chunk(i)` (i < 8), as fp32 (each square and partial sum rounded:
// relative error < 100 u, covered by error_model.cpp's safety factor in
// amb_t2e). U chunks in flight at a time: the sum's order, and so its bits,
// do not depend on U.
template <int U, typename Chunk>
__device__ __forceinline__ float seg_energy_lowreg(Chunk chunk)
{
    f2 a = {0.f, 0.f}, b = {0.f, 0.f};
#pragma unroll U
    for (int i = 0; i < 8; ++i) {
        const u32x4 d = chunk(i);
        const unsigned d4[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f2 x = {(float)(int)(short)(d4[q] & 0xFFFFu), (float)((int)d4[q] >> 16)};
            if (q & 1) b = __builtin_elementwise_fma(x, x, b);
            else a = __builtin_elementwise_fma(x, x, a);
        }
    }
    return (a.x + a.y) + (b.x + b.y);
}

// All 8 chunks in flight.
template <typename Chunk>
__device__ __forceinline__ float seg_energy(Chunk chunk)
{
    return seg_energy_lowreg<8>(chunk);
}

// A serial sum one chunk at a time (4 VGPRs of samples live instead of 32:
// for rare paths inside kernels at their VGPR limit)
template <typename Chunk>
__device__ __forceinline__ float seg_energy_serial(Chunk chunk)
{
    float e = 0.f;
#pragma unroll 1
    for (int i = 0; i < 8; ++i) {
        const u32x4 d = chunk(i);
        const unsigned d4[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float x = (float)(short)((d4[q >> 1] >> (16 * (q & 1))) & 0xFFFFu);
            e = __builtin_fmaf(x, x, e);
        }
    }
    return e;
}

// Tile-group index of this block. Blocks are dealt round-robin to the 8 XCDs
// (MI355X_MICROARCH.md §Workgroup dispatch), so with the swizzle each XCD
// walks one contiguous 1/8 of the tiles and every output line is written by a
// single XCD's L2. Placement only affects speed, never correctness.
__device__ __forceinline__ long long tile_block(int swz)
{
    const long long b = blockIdx.x, nb = gridDim.x;
    if (!swz) return b;
    const long long per = nb / 8, full = per * 8;
    if (b >= full) return b;
    return (b % 8) * per + b / 8;
}

// Write-back bursts (round 3), at the end of a Goertzel-family
// tile kernel. A batch whose outputs are more than the XCDs' L2s hold dirty
// (8-FSK: 33 MiB) runs as one launch in which the last block of every
// 1/wb_bursts of an XCD's swizzled blocks (its wave 0, after its stores)
// writes that XCD's L2 back with an agent-scope release, so the output lines
// leave in a few bursts instead of trickling out between the input's reads;
// the launch slices this replaces paid a drain and a ramp per slice.
__device__ __forceinline__ void wb_burst(int wb_bursts)
{
    if (wb_bursts <= 0 || threadIdx.x >= 64) return;
    const long long b = blockIdx.x, per = gridDim.x / 8, seg = per / wb_bursts;
    if (seg > 0 && b < per * 8 && (b / 8) % seg == seg - 1)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
}

}  // namespace fskd
