// rescue_ops.h — the decision rescue's double-precision steps, each written
// once. Device only. rescue.hip is built from these; the
// in-kernel rescues (rescue_rows.h, rescue_fft.h) call them where the
// detector kernels' machine code allows and name them where it does not.
// Every sum's order and every operand order here is part of the contract
// ("every symbol equals the double oracle's, bit for bit"): contraction is off
// inside each helper, and nothing is reassociated.
#pragma once
#include "lane_ops.h"

namespace fskd {

// int16 sample `half` (0: low, 1: high) of a dword of packed samples — the
// oracle's x[i] (oracle/fsk_oracle.c goertzel_window_d, `(double)x[i]`).
// Sample i of a 16-byte chunk's dwords d4 is sample16(d4[i >> 1], i & 1).
__device__ __forceinline__ short sample16(unsigned dword, int half)
{
    return (short)((dword >> (16 * half)) & 0xFFFFu);
}

// One step of the definition's recurrence, `s = x + c s1 - s2; s2 = s1; s1 =
// s` (oracle/fsk_oracle.c goertzel_window_d's inner loop; error_model.cpp
// chain_double): product, sum and difference each rounded on its own.
__device__ __forceinline__ void chain_step_d(double x, double c, double &s1, double &s2)
{
#pragma clang fp contract(off)
    double s = x + c * s1;
    s = s - s2;
    s2 = s1;
    s1 = s;
}

// The recurrence over the 8 samples of a 16-byte chunk, in order: 8
// iterations of goertzel_window_d's inner loop.
__device__ __forceinline__ void exact_step8(const unsigned (&d4)[4], double c, double &s1, double &s2)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 8; ++i) chain_step_d((double)sample16(d4[i >> 1], i & 1), c, s1, s2);
}

// The definition's power, `p = s1 * s1 + s2 * s2 - c[t] * s1 * s2`
// (goertzel_window_d), in C's evaluation order: (s1^2 + s2^2) - ((c s1) s2).
__device__ __forceinline__ double exact_power(double c, double s1, double s2)
{
#pragma clang fp contract(off)
    const double a = s1 * s1 + s2 * s2;
    const double b = c * s1;
    return a - b * s2;
}

// Sum over the 16 lanes of a row (n = 1024 windows), every lane the same total.
__device__ __forceinline__ float row_sum16(float v)
{
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, true));
    return v;
}

// The same tree in double (the rescue's pass 0): each stage's partner by DPP
// (two 32-bit moves) instead of __shfl_xor's ds_bpermute round trips through
// the LDS crossbar. Bit-identical to the xor butterfly: after each stage the
// lanes of a group hold one value (a + b == b + a), so any lane of the
// partner group is the partner.
template <int C>
__device__ __forceinline__ double dpp_d(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)b, C, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(b >> 32), C, 0xF, 0xF, true);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The window sum of error_model.cpp's WindowAcc over a row's 16 segments
// (levels = 4), as a xor butterfly.
__device__ __forceinline__ double row_sum16d(double v)
{
    v += dpp_d<0xB1>(v);
    v += dpp_d<0x4E>(v);
    v += dpp_d<0x141>(v);
    v += dpp_d<0x140>(v);
    return v;
}

// Pass 0's power of one tone from a row's rotated parts (re, im this lane's):
// the row sums, then re^2 + im^2 (error_model.cpp first_pass_rho's WindowAcc
// and power).
__device__ __forceinline__ double pass0_power(double re, double im)
{
#pragma clang fp contract(off)
    re = row_sum16d(re);
    im = row_sum16d(im);
    return re * re + im * im;
}

// The lane's segment end state (s1, s2) of a real chain rotated into the
// window's phase by r = {Ar, Ai, Br, Bi} (rot64 + 4 (16 t + seg)): re = Ar s1 -
// Br s2, im = Ai s1 - Bi s2, both products and the difference rounded
// (error_model.cpp rotate2).
__device__ __forceinline__ void pass0_rotate(const double *r, double s1, double s2, double &re, double &im)
{
#pragma clang fp contract(off)
    re = r[0] * s1;
    im = r[1] * s1;
    re = re - r[2] * s2;
    im = im - r[3] * s2;
}

// Pass 0's head: pass0_rotate, then pass0_power (error_model.cpp
// first_pass_rho and first_pass_fold_rho after their chain_double).
__device__ __forceinline__ double pass0_head(const double *r, double s1, double s2)
{
    double re, im;
    pass0_rotate(r, s1, s2, re, im);
    return pass0_power(re, im);
}

// Pass 0 by the fold: one 16-byte chunk (samples 128 m + 8 seg + i, i < 8)
// added into the lane's folded samples xf[i], exact integers
// (error_model.cpp first_pass_fold_rho's xf).
__device__ __forceinline__ void fold_add8(const unsigned (&d4)[4], int (&xf)[8])
{
#pragma unroll
    for (int i = 0; i < 8; ++i) xf[i] += (int)sample16(d4[i >> 1], i & 1);
}

// Running argmax with its runner-up, ties to the lowest tone (goertzel_window_d's
// `if (p > best)`, plus the second power the margin test needs). Start from
// best = second = -1, arg = 0.
__device__ __forceinline__ void top2_update(double pk, int k, double &best, double &second, int &arg)
{
    if (pk > best) {
        second = best;
        best = pk;
        arg = k;
    } else if (pk > second) {
        second = pk;
    }
}

// Pass 0's margin test (error_model.cpp error_model's t2e64 = 16 rho_first^2):
// the row stays ambiguous unless margin^2 >= t2e64 E P_max and P_max is above
// the floor t2e64 E / 16; e is this lane's fp32 sum x^2 (E: the row's sum,
// within 1e-5; the host's t2e64 carries (1 + 1e-3)).
__device__ __forceinline__ bool pass0_still(double t2e64, float e, double best, double second)
{
#pragma clang fp contract(off)
    const double cth = t2e64 * (double)row_sum16(e), dm = best - second;
    return !(best > 0.0) || dm * dm < cth * best || 16.0 * best < cth;
}

// x_lo^2 + x_hi^2 of one dword of packed samples, exact by v_dot2_i32_i16
// (clamped: only (-32768, -32768) saturates, to 2^31 - 1), converted to fp32:
// one term of pass 0's energy E (error_model.cpp allows E 100 u). The callers
// keep their own sum orders (the fp32 bits of E set pass 0's threshold).
typedef short i16x2_dot __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float dot_sq2(unsigned dword)
{
    const i16x2_dot s = __builtin_bit_cast(i16x2_dot, dword);
    return (float)__builtin_amdgcn_sdot2(s, s, 0, true);
}

}  // namespace fskd
