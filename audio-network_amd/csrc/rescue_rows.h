// rescue_rows.h — the decision rescue inside the direct Goertzel-family
// detector kernels (goertzel.hip, fold.hip, residue.hip).
// Device only. The steps are rescue_ops.h's; where one stands inline here
// instead of calling its helper, the detector kernels' machine code depends
// on it (scripts/kernel_isa_diff.py) and a comment names the helper.
#pragma once
#include "kernel_ops.h"

namespace fskd {

// In-kernel decision rescue of a wave's flagged windows, each by its 16-lane
// row (n = 1024; round 3 for the 2-FSK plain bank, round 4 every direct
// Goertzel-family kernel at n = 1024). Two passes of one loop (one copy of
// the code, so the detector's VGPR budget pays for one):
//  pass 0 (round 4, when t2e64 > 0): the row's K powers in double, computed
//    the way the fp32 plain bank computes them — lane seg runs every tone's
//    recurrence over its own 64 samples, rotates its end state into the
//    window's phase (rot64) and the row sums — K x 64 double steps per lane
//    on all 16 lanes, instead of one 1024-step chain per tone on K lanes
//    (~10x fewer wave instructions at K = 2). These powers are not the
//    oracle's bits, but |sqrt P_0 - sigma P_ref| <= rho_first sqrt(E) (its own
//    rounding and the oracle's, derived by error_model.cpp from both
//    operation sequences; checked by tests/test_rescue_model64.py), so where
//    their top-2 margin satisfies margin^2 >= t2e64 E P_max (t2e64 = 16
//    rho_first^2) the argmax is the oracle's and the row is decided here (its
//    magnitudes: these powers rounded to fp32, within the bound of the
//    oracle's). Rows inside that band (exact ties; margins within ~1e-10 of
//    P_max) go on to
//  pass 1: lane seg < K runs tone seg's recurrence in double over the
//    window's 1024 samples with exactly rescue_kernel's operations and order
//    (so exactly oracle/fsk_oracle.c's: contraction off); the row's argmax
//    (ties to the lowest tone) replaces the symbol, and the powers (rounded
//    to fp32) the magnitudes, bit-identical to the oracle's.
// chunk(q) returns the window's 16-byte chunk q (samples 8q .. 8q + 7) from
// wherever the kernel holds the tile (its LDS slice: no global round trip).
// Every lane of the wave calls it (the shuffles); rows with amb_row false
// change nothing. The detector leaves the symbol and magnitudes of a flagged
// row to this function (no second store).
// Pass 0 by the fold (FOLD: fold detector plans, every tone on a multiple of
// 8 bins; round 5): lane seg sums the window's samples
// 128 m + 8 seg + i over m < 8 (exact integers: the folded samples 8 seg ..
// 8 seg + 7 of the window folded to 128), then per tone an 8-step double
// chain at the exact bin, the rotation (rot64: the fold tables, plan.h
// fold64), the row sum and the power; the margin test as pass 0 above (t2e64
// derived for this sequence, error_model.cpp first_pass_fold_rho). 8x fewer
// double steps than 64 raw samples per lane per tone. Returns amb_row after
// it (the rows left to the exact chains).
// x_lo^2 + x_hi^2 of 4 dwords (8 int16 samples): exact per dword by
// v_dot2_i32_i16 (clamped, only (-32768, -32768) saturates, to 2^31 - 1),
// converted and summed in fp32 (pass 0's energy: error_model.cpp allows E
// 100 u, this is < 36 u over a lane's 64 samples)
__device__ __forceinline__ float dot_energy4(const unsigned (&d4)[4])
{
    float e = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) e += dot_sq2(d4[c]);
    return e;
}

template <int K, typename Chunk>
__device__ __forceinline__ bool rescue_rows_fold0(const GoertzelParams &p, long long w, int seg,
                                                  bool amb_row, Chunk chunk)
{
#pragma clang fp contract(off)
    // opaque here: no address built from seg is hoisted into the detector's
    // loop (where it would hold VGPRs across every tile)
    asm volatile("" : "+v"(seg));
    int xf[8];
    float e = 0.f;  // the lane's 64 raw samples' sum x^2 (any partition of the window)
#pragma unroll
    for (int i = 0; i < 8; ++i) xf[i] = 0;
#pragma unroll 1
    for (int m = 0; m < 8; ++m) {
        const u32x4 d = chunk(16 * m + seg);
        const unsigned d4[4] = {d.x, d.y, d.z, d.w};
        fold_add8(d4, xf);
        e += dot_energy4(d4);
    }
    double best = -1.0, second = -1.0;
    int arg = 0;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        int ci = 64 * K + k;
        asm volatile("" : "+v"(ci));  // a vector load (as scalar, SGPR spills at large K)
        const double c = p.rot64[ci];
        double s1 = 0.0, s2 = 0.0;
        // each sample converted at its step (scheduled together, the 8
        // doubles raised the fold kernels' VGPR peak)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            chain_step_d((double)xf[i], c, s1, s2);
            __builtin_amdgcn_sched_barrier(0);
        }
        const double2 A = *reinterpret_cast<const double2 *>(p.rot64 + 4 * (k * 16 + seg));
        const double2 B = *reinterpret_cast<const double2 *>(p.rot64 + 4 * (k * 16 + seg) + 2);
        double re = A.x * s1, im = A.y * s1;
        re = re - B.x * s2;
        im = im - B.y * s2;
        const double pk = pass0_power(re, im);
        // (rescue_ops.h top2_update, inline: through the helper the detector kernels' machine code changes)
        if (pk > best) {
            second = best;
            best = pk;
            arg = k;
        } else if (pk > second) {
            second = pk;
        }
        if (k == seg && amb_row && p.mag) p.mag[w * K + seg] = (float)pk;
    }
    // (rescue_ops.h pass0_still, inline: through the helper the detector kernels' machine code changes)
    const double cth = p.t2e64 * (double)row_sum16(e), dm = best - second;
    const bool still = !(best > 0.0) || dm * dm < cth * best || 16.0 * best < cth;
    if (amb_row && !still && seg == 0) p.sym[w] = (uint8_t)arg;
    return amb_row && still;
}

// FOLD: 0 = pass 0 by segments, 1 = by the fold (fold kernels), 2 = as the
// plan says at run time (p.fold64: plain-bank plans on multiples of 8 bins)
template <int K, int FOLD = 0, typename Chunk>
__device__ __forceinline__ void rescue_rows(const GoertzelParams &p, long long w, int seg, int lane,
                                            bool amb_row, Chunk chunk)
{
#pragma clang fp contract(off)
    int first = p.t2e64 > 0.0 ? 0 : 1;
    if constexpr (FOLD != 0) {
        if (first == 0 && (FOLD == 1 || p.fold64)) {
            amb_row = rescue_rows_fold0<K>(p, w, seg, amb_row, chunk);
            if (__ballot(amb_row) == 0) return;
            first = 1;
        }
    }
#pragma unroll 1
    for (int pass = first; pass < 2; ++pass) {
        const bool exact = pass == 1;
        const bool run = exact ? amb_row && seg < K : true;  // lanes that run chains
        const int q0 = exact ? 0 : 8 * seg, q1 = exact ? 128 : 8 * seg + 8;
        double best = -1.0, second = -1.0, mine = 0.0;
        float e = 0.f;  // pass 0: the lane's sum x^2
        int arg = 0;
#pragma unroll 1
        for (int t = 0; t < (exact ? 1 : K); ++t) {
            const int k = exact ? seg : t;
            // pass 0's coefficient, or the oracle's rcoef[k] (exact), per lane
            const double c = p.rot64[(exact ? 65 : 64) * K + (k < K ? k : 0)];
            double s1 = 0.0, s2 = 0.0;
            if (run) {
#pragma unroll 1
                for (int q = q0; q < q1; ++q) {
                    const u32x4 d = chunk(q);
                    const unsigned d4[4] = {d.x, d.y, d.z, d.w};
                    if (!exact && t == 0) e += dot_energy4(d4);
                    // (rescue_ops.h exact_step8, and exact_power below, inline:
                    // through the helpers the detector kernels' machine code changes)
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const double x = (double)sample16(d4[i >> 1], i & 1);
                        double s = x + c * s1;
                        s = s - s2;
                        s2 = s1;
                        s1 = s;
                    }
                }
            }
            if (exact) {
                const double a = s1 * s1 + s2 * s2;
                const double b = c * s1;
                mine = run ? a - b * s2 : 0.0;
            } else {
                // the rotation's loads after the chain (an offset that depends
                // on its result): hoisted above it they hold 8 VGPRs through it
                // (and B's after A's products: 4 VGPRs of table live at a time)
                int ro = 4 * (k * 16 + seg);
                asm volatile("" : "+v"(ro) : "v"(s1));
                const double2 A = *reinterpret_cast<const double2 *>(p.rot64 + ro);
                double re = A.x * s1, im = A.y * s1;
                asm volatile("" : "+v"(ro) : "v"(re), "v"(im));
                const double2 B = *reinterpret_cast<const double2 *>(p.rot64 + ro + 2);
                re = re - B.x * s2;
                im = im - B.y * s2;
                const double pk = pass0_power(re, im);
                // (rescue_ops.h top2_update, inline: through the helper the
                // detector kernels' machine code changes)
                if (pk > best) {
                    second = best;
                    best = pk;
                    arg = k;
                } else if (pk > second) {
                    second = pk;
                }
                // the row's magnitudes now (pass 1 rewrites those of the rows
                // it takes over): no register holds them across the loop
                if (k == seg && amb_row && p.mag) p.mag[w * K + seg] = (float)pk;
            }
        }
        bool still = false;
        if (exact) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double pk = __shfl(mine, (lane & 48) + k);
                if (pk > best) {
                    best = pk;
                    arg = k;
                }
            }
        } else {
            // stage threshold^2 = t2e64 E P_max, E the row's sum x^2 (fp32,
            // within 1e-5: the host's t2e64 carries (1 + 1e-3))
            // (rescue_ops.h pass0_still, inline: through the helper the
            // detector kernels' machine code changes)
            const double cth = p.t2e64 * (double)row_sum16(e), dm = best - second;
            still = !(best > 0.0) || dm * dm < cth * best || 16.0 * best < cth;
        }
        if (amb_row && !still) {
            if (seg == 0) p.sym[w] = (uint8_t)arg;
            if (exact && p.mag && seg < K) p.mag[w * K + seg] = (float)mine;
        }
        amb_row = amb_row && still;
        if (__ballot(amb_row) == 0) break;
    }
}

}  // namespace fskd
