/*
 * soft_ops.h — the one device copy of a row's soft value at an air position (include/demod.h "coded frames"),
 * shared by the Viterbi decode's soft pass (frames_fec.hip) and the erasure mask's producer
 * (frames_erasures.hip). demod_fec.c's demod_soft_bits restates it on the host.
 */
#ifndef FSKD_SOFT_OPS_H
#define FSKD_SOFT_OPS_H

namespace fskd {

// Air value a = j bits + b of a row whose symbol 0 of the word sits at window bw: the K powers of window bw +
// (L + j) R, the largest with bit b clear and with bit b set (each from the lowest such tone, replaced by a
// strictly greater one alone), then one double expression. A window at or past n_windows is an erasure (0) and
// is not read. The caller holds a below N bits.
static __device__ __forceinline__ int soft_air_value(const float *mag, unsigned n_windows, unsigned k,
                                                     unsigned bits, unsigned sync_len, unsigned phases,
                                                     unsigned long long bw, unsigned a)
{
    const unsigned j = a / bits, b = a - j * bits;
    const unsigned long long w = bw + ((unsigned long long)sync_len + j) * phases;
    if (w >= n_windows) return 0;
    const float *P = mag + (size_t)w * k;
    const unsigned mask = 1u << (bits - 1u - b);
    float a0 = P[0], a1 = P[mask];
    for (unsigned i = 1; i < k; ++i) {
        const float f = P[i];
        if (i & mask) {
            if (f > a1) a1 = f;
        } else if (f > a0) {
            a0 = f;
        }
    }
    const double d = (double)a0 - (double)a1, s = fabs((double)a0) + fabs((double)a1);
    return (s > 0.0 && s <= 1.7976931348623157e308) ? (int)rint(127.0 * d / s) : 0;
}

}  // namespace fskd

#endif
