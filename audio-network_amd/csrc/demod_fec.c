/*
 * demod_fec.c — the host side of the coded frame (include/demod.h "coded
 * frames", DESIGN.md §4.9 "Coded frames"): the constraint-length-7, rate-1/2
 * convolutional encoder (0171/0133) over a checked frame's bytes, the soft
 * values of one window's tone powers, and the soft-decision Viterbi decoder
 * the device (frames_fec.hip) is held to, bit for bit; each also in the
 * punctured and interleaved modes, through the map of fec_map.h (the
 * demod_fec_* functions; the older ones are their fec == 1 case). Integer arithmetic
 * apart from one double expression per soft value. Pure host work, no device.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "frame_shape.h"

#define FEC_G0 0171u
#define FEC_G1 0133u
#define FEC_STATES 64

static unsigned parity7(unsigned v)
{
    v ^= v >> 4;
    v ^= v >> 2;
    v ^= v >> 1;
    return v & 1u;
}

/* The span of a frame in a mode with the convolutional code (frame_shape.h), in symbols of `bits` bits, with
 * its T and Nt; or the negative code of demod_checked_frame_size. */
static long long coded_span(size_t len, int len_bytes, int crc, int bits, unsigned fec, unsigned *T, unsigned *Nt)
{
    const long long n = demod_checked_frame_size(len, len_bytes, crc);
    if (n < 0) return n;
    return (long long)frame_air_symbols((unsigned)len, (unsigned)len_bytes, (unsigned)frame_crc_bytes(crc),
                                        (unsigned)bits, rs_mode_conv(fec), rs_parity(fec), T, Nt);
}

long long demod_coded_frame_steps(size_t len, int len_bytes, int crc)
{
    unsigned T, Nt;
    const long long rc = coded_span(len, len_bytes, crc, 1, DEMOD_FEC_CONV_K7, &T, &Nt);
    return rc < 0 ? rc : (long long)T;
}

/* a mode with the convolutional code: one of the six, with or without a parity flag */
static int conv_mode_valid(int fec)
{
    return rs_mode_valid((unsigned)fec) && rs_mode_conv((unsigned)fec) != 0u;
}

long long demod_fec_air_index(int fec, size_t m)
{
    if (!conv_mode_valid(fec) || m > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    const unsigned a = fec_air_of_mother(rs_mode_conv((unsigned)fec), (unsigned)m);
    return a == FEC_MAP_NONE ? -1 : (long long)a;
}

long long demod_fec_frame_symbols(size_t len, int len_bytes, int crc, int bits, int fec)
{
    unsigned T, Nt;
    if (!conv_mode_valid(fec)) return DEMOD_BAD_ARG;
    const int ok = bits >= 1 && bits <= 4;   /* refused behind what the frame's size refuses */
    const long long sp = coded_span(len, len_bytes, crc, ok ? bits : 1, (unsigned)fec, &T, &Nt);
    return sp < 0 || ok ? sp : DEMOD_BAD_ARG;
}

long long demod_coded_frame_symbols(size_t len, int len_bytes, int crc, int bits)
{
    return demod_fec_frame_symbols(len, len_bytes, crc, bits, DEMOD_FEC_CONV_K7);
}

int demod_fec_frame_encode(const uint8_t *data, size_t len, int len_bytes, int crc, int fec, uint8_t *out,
                           size_t cap)
{
    unsigned T, Nt;
    if (!conv_mode_valid(fec)) return DEMOD_BAD_ARG;
    const long long Na = coded_span(len, len_bytes, crc, 1, (unsigned)fec, &T, &Nt);   /* one bit a symbol: Na */
    if (Na < 0) return (int)Na;
    if ((!data && len) || !out) return DEMOD_BAD_ARG;
    const unsigned P = rs_parity((unsigned)fec), conv = rs_mode_conv((unsigned)fec);
    const size_t need = (size_t)(Na + 7) / 8;
    if (need > cap) return DEMOD_BUFFER_TOO_SMALL;
    uint8_t info[2 + DEMOD_MAX_FRAME_PAYLOAD + 4 + 19 * RS_MAX_PARITY];   /* the longest n' */
    int n = demod_checked_frame_encode(data, len, len_bytes, crc, info, sizeof(info));
    if (n < 0) return n;
    rs_frame_protect(info, (unsigned)n, P);
    n = (int)rs_frame_bytes((unsigned)n, P);
    memset(out, 0, need);
    unsigned reg = 0;
    for (long long t = 0; t < (long long)T; ++t) {
        const unsigned u = t < 8 * (long long)n ? (info[t >> 3] >> (7 - (t & 7))) & 1u : 0u;
        reg = ((reg << 1) | u) & 0x7Fu;
        for (unsigned v = 0; v < 2; ++v) {
            const unsigned a = fec_air_of_mother(conv, 2u * (unsigned)t + v);
            if (a == FEC_MAP_NONE) continue;   /* punctured */
            out[a >> 3] |= (uint8_t)(parity7(reg & (v ? FEC_G1 : FEC_G0)) << (7 - (a & 7)));
        }
    }
    return (int)need;
}

int demod_coded_frame_encode(const uint8_t *data, size_t len, int len_bytes, int crc, uint8_t *out,
                             size_t cap)
{
    return demod_fec_frame_encode(data, len, len_bytes, crc, DEMOD_FEC_CONV_K7, out, cap);
}

long long demod_fec_row_bytes(size_t frame_symbols, int bits, int len_bytes, int fec)
{
    if (bits < 1 || bits > 4 || frame_symbols > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    if (!conv_mode_valid(fec) || (len_bytes != 1 && len_bytes != 2)) return DEMOD_BAD_ARG;
    const long long St = (long long)frame_row_steps(rs_mode_conv((unsigned)fec), frame_symbols * (size_t)bits);
    return St < 8 * len_bytes + DEMOD_FEC_DEPTH ? DEMOD_BAD_ARG : (St - 6) / 8;
}

long long demod_coded_row_bytes(size_t frame_symbols, int bits, int len_bytes)
{
    return demod_fec_row_bytes(frame_symbols, bits, len_bytes, DEMOD_FEC_CONV_K7);
}

int demod_soft_bits(const float *powers, uint32_t k, int8_t *soft)
{
    if (!powers || !soft || k < 2 || k > DEMOD_MAX_TONES || (k & (k - 1)) != 0) return DEMOD_BAD_ARG;
    const int bits = demod_bits_per_symbol(k);
    for (int b = 0; b < bits; ++b) {
        const uint32_t m = 1u << (bits - 1 - b);
        /* each maximum from the lowest such tone, replaced by a strictly greater one alone */
        float a0 = powers[0], a1 = powers[m];
        for (uint32_t i = 1; i < k; ++i) {
            if (i & m) {
                if (powers[i] > a1) a1 = powers[i];
            } else if (powers[i] > a0) {
                a0 = powers[i];
            }
        }
        const double d = (double)a0 - (double)a1, s = fabs((double)a0) + fabs((double)a1);
        soft[b] = (s > 0.0 && s <= 1.7976931348623157e308) ? (int8_t)(int)rint(127.0 * d / s) : 0;
    }
    return bits;
}

int demod_soft_erasures(const int8_t *soft, size_t n_soft, int level, uint64_t *erase, size_t row_bytes)
{
    if (!soft || !erase || ((uintptr_t)erase & 7) != 0 || level < 1 || level > 127) return DEMOD_BAD_ARG;
    if (row_bytes == 0 || row_bytes > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    const unsigned Wm = rs_mask_words((unsigned)row_bytes);
    memset(erase, 0, (size_t)Wm * sizeof(uint64_t));
    for (size_t b = 0; b < row_bytes; ++b) {
        int least = 128;
        for (size_t m = 8 * b; m < 8 * b + 8; ++m) {
            const int q = m < n_soft ? soft[m] : 0, a = q < 0 ? -q : q;
            if (a < least) least = a;
        }
        if (least < level) erase[b >> 6] |= (uint64_t)1 << (b & 63u);
    }
    return (int)Wm;
}

/* u_t of steps t_end-1 .. 0 from state s at step t_end, into bits[] (one byte a bit) */
static void trace_back(const uint64_t *surv, size_t t_end, unsigned s, uint8_t *bits)
{
    for (size_t t = t_end; t-- > 0;) {
        bits[t] = (uint8_t)(s & 1u);
        s = (s >> 1) | ((unsigned)((surv[t] >> s) & 1u) << 5);
    }
}

static void forward(const int8_t *soft, size_t t_from, size_t t_to, int32_t *M, uint64_t *surv)
{
    for (size_t t = t_from; t < t_to; ++t) {
        const int32_t q0 = soft[2 * t], q1 = soft[2 * t + 1];
        int32_t next[FEC_STATES];
        uint64_t word = 0;
        for (unsigned s = 0; s < FEC_STATES; ++s) {
            const unsigned p0 = s >> 1, p1 = p0 | 32u;
            int32_t sum[2];
            for (int j = 0; j < 2; ++j) {
                const unsigned reg = (((j ? p1 : p0) << 1) | (s & 1u)) & 0x7Fu;
                const int32_t bm = (parity7(reg & FEC_G0) ? -q0 : q0) + (parity7(reg & FEC_G1) ? -q1 : q1);
                sum[j] = M[j ? p1 : p0] + bm;
            }
            const int d = sum[1] > sum[0];
            next[s] = d ? sum[1] : sum[0];
            word |= (uint64_t)d << s;
        }
        memcpy(M, next, sizeof(next));
        surv[t] = word;
    }
}

/* the decoder on the 2 St trellis soft values q (punctured positions 0) of a row of shape z, into its Bd bytes */
static int trellis_decode(const int8_t *soft, const struct frame_shape *z, uint8_t *row,
                          demod_frame_decode_t *decode)
{
    const size_t St = z->steps, h = (size_t)z->len_bytes, c = (size_t)z->crc_bytes, max_len = z->max_len;
    const unsigned P = (unsigned)z->parity;
    const size_t t0 = 8 * h + DEMOD_FEC_DEPTH;
    uint64_t *surv = (uint64_t *)malloc(St * sizeof(uint64_t));
    uint8_t *bits = (uint8_t *)malloc(St);
    if (!surv || !bits) {
        free(surv);
        free(bits);
        return DEMOD_ALLOC_FAIL;
    }
    int32_t M[FEC_STATES];
    M[0] = 0;
    for (unsigned s = 1; s < FEC_STATES; ++s) M[s] = -(1 << 28);
    forward(soft, 0, t0, M, surv);
    unsigned best = 0;
    for (unsigned s = 1; s < FEC_STATES; ++s)
        if (M[s] > M[best]) best = s;
    trace_back(surv, t0, best, bits);
    size_t len = 0;
    for (size_t t = 0; t < 8 * h; ++t) len = (len << 1) | bits[t];
    int written;
    if (len > max_len) {
        decode->length = (uint32_t)len;
        decode->metric = 0;
        decode->status = DEMOD_DECODE_BAD_LENGTH;
        decode->steps = 0;
        for (size_t b = 0; b < h; ++b) row[b] = (uint8_t)(len >> (8 * (h - 1 - b)));
        written = (int)h;
    } else {
        const size_t n = rs_frame_bytes((unsigned)(h + len + c), P);
        const size_t T = 8 * n + 6 > t0 ? 8 * n + 6 : t0;   /* <= St: n <= Bd */
        forward(soft, t0, T, M, surv);
        trace_back(surv, T, 0, bits);
        for (size_t b = 0; b < n; ++b) {
            unsigned v = 0;
            for (int i = 0; i < 8; ++i) v = (v << 1) | bits[8 * b + i];
            row[b] = (uint8_t)v;
        }
        decode->length = (uint32_t)len;
        decode->metric = M[0];
        decode->status = DEMOD_DECODE_OK;
        decode->steps = (uint32_t)T;
        written = (int)n;
    }
    free(surv);
    free(bits);
    return written;
}

int demod_fec_frame_decode(const int8_t *soft, size_t n_soft, int len_bytes, int crc, int fec, uint8_t *row,
                           size_t cap, demod_frame_decode_t *decode)
{
    struct frame_shape z;   /* of a row of n_soft one-bit symbols */
    if (!soft || !row || !decode || !conv_mode_valid(fec)) return DEMOD_BAD_ARG;
    if (frame_shape_fill(&z, 1, 1, n_soft, len_bytes, crc, fec)) return DEMOD_BAD_ARG;
    if (cap < z.row_bytes) return DEMOD_BUFFER_TOO_SMALL;
    const unsigned conv = (unsigned)z.fec;
    const size_t St = z.steps;
    if (!fec_mode_mapped(conv)) return trellis_decode(soft, &z, row, decode);
    /* the trellis's order: q_m from air position a(m), 0 where m is punctured */
    int8_t *q = (int8_t *)malloc(2 * St);
    if (!q) return DEMOD_ALLOC_FAIL;
    for (size_t m = 0; m < 2 * St; ++m) {
        const unsigned a = fec_air_of_mother(conv, (unsigned)m);   /* < Cu <= n_soft */
        q[m] = a == FEC_MAP_NONE ? 0 : soft[a];
    }
    const int rc = trellis_decode(q, &z, row, decode);
    free(q);
    return rc;
}

int demod_coded_frame_decode(const int8_t *soft, size_t n_soft, int len_bytes, int crc, uint8_t *row,
                             size_t cap, demod_frame_decode_t *decode)
{
    return demod_fec_frame_decode(soft, n_soft, len_bytes, crc, DEMOD_FEC_CONV_K7, row, cap, decode);
}
