// crc_ops.h — device helpers of the lane-split CRC that frames_check.hip (the
// receiver's check) and frames_tx.hip (the transmitter's write) share. The
// register and P sit in the top `width` bits of a 32-bit word, so CRC-16 and
// CRC-32 share every line; by linearity
//     crc(init, A || B) = crc(init, A) x^(8 |B|) + crc(0, B)  mod P
// each lane runs the byte table over its own chunk, multiplies its register by
// x^(8 bytes after its chunk) and the wave XORs the 64 registers.
#pragma once
#include "demod_internal.h"

namespace fskd {

// r(x) x mod P; the register and P in the top `width` bits
static __device__ __forceinline__ unsigned crc_xtime(unsigned r, unsigned poly)
{
    return (r << 1) ^ ((r >> 31) ? poly : 0u);
}

// The 256-entry byte table (crc_xtime eight times over t << 24) into s_tab by
// a workgroup of 256 threads, one entry each; the caller's barrier follows.
static __device__ __forceinline__ void crc_byte_table(unsigned *s_tab, unsigned poly)
{
    const int t = threadIdx.x;
    unsigned r = (unsigned)t << 24;
    for (int b = 0; b < 8; ++b) r = crc_xtime(r, poly);
    s_tab[t] = r;
}

// a(x) b(x) mod P by Horner over b's WIDTH coefficients, highest first; no
// branches. Unrolled by 8 only, and its caller's loop not at all: a wave runs
// this code once, and straight-line code costs more to fetch than it saves.
template <int WIDTH>
static __device__ __forceinline__ unsigned crc_mul(unsigned a, unsigned b, unsigned poly)
{
    unsigned r = 0;
#pragma unroll 8
    for (int i = 0; i < WIDTH; ++i) {
        r = (r << 1) ^ (poly & (unsigned)((int)r >> 31)) ^ (a & (unsigned)((int)b >> 31));
        b <<= 1;
    }
    return r;
}

// The wave's CRC register over row[0 .. n): lane `lane` of 64 takes its
// contiguous chunk of ceil(n / 64) bytes, lane 0 from init and the others from
// 0. tab is the 256-entry byte table (crc_byte_table),
// xpow8[j] = x^(8 2^j) mod P from the host. The same value in every lane.
template <int WIDTH>
static __device__ __forceinline__ unsigned crc_wave(const uint8_t *row, unsigned n, int lane, unsigned init,
                                                    unsigned poly, const unsigned *xpow8, const unsigned *tab)
{
    const unsigned chunk = (n + 63) / 64;
    const unsigned lo = (unsigned)lane * chunk < n ? (unsigned)lane * chunk : n;
    const unsigned hi = lo + chunk < n ? lo + chunk : n;
    unsigned reg = lane == 0 ? init : 0u;
    for (unsigned b = lo; b < hi; ++b) reg = (reg << 8) ^ tab[(reg >> 24) ^ row[b]];
    if (reg != 0 && hi < n) {
        // times x^(8 (n - hi)): square-and-multiply, the squares x^(8 2^j) from the host
        const unsigned after = n - hi;
#pragma unroll 1
        for (int j = 0; j < kCrcPowBits && (after >> j) != 0; ++j)
            if ((after >> j) & 1u) reg = crc_mul<WIDTH>(reg, xpow8[j], poly);
    }
    for (int d = 32; d > 0; d >>= 1) reg ^= __shfl_xor(reg, d);
    return reg;
}

}  // namespace fskd
