/*
 * rs_ops.h — the one copy of the Reed-Solomon outer code's field arithmetic
 * and frame layout (include/demod.h "Reed-Solomon outer code"), shared by
 * frames_rs.hip, the host entry points and the host C (demod_rs.c,
 * demod_fec.c). Plain integer code that compiles for both.
 *
 *  field     GF(2^8), reduction polynomial 0x11D, alpha = 2
 *  code      P = 16 or 32 parity bytes, g(x) = prod_{i<P} (x - alpha^i);
 *            systematic, the message's first byte the highest coefficient,
 *            shortened: the missing leading symbols are 0 and never sent
 *  frame     F = len || data || CRC of n bytes is cut into D = ceil(n / (255 -
 *            P)) codewords byte by byte: codeword j holds F[j], F[j + D], ..
 *            (k_j = ceil((n - j) / D) bytes) and the parity bytes n + i D + j,
 *            i < P. n' = n + D P.
 *  erasures  the level's bits of `fec`, the mask's addressing and the flag of a
 *            codeword's symbol (include/demod.h "erasure decoding")
 */
#ifndef FSKD_RS_OPS_H
#define FSKD_RS_OPS_H

#include <stdint.h>

#include "fec_map.h"

#define RS_OPS_FN FEC_MAP_FN

#define RS_FLAG_16 0x100u
#define RS_FLAG_32 0x200u
#define RS_MAX_PARITY 32
#define RS_MAX_T 16
#define RS_MAX_ERRATA RS_MAX_PARITY      /* f erasures and e errors, 2 e + f <= P: at most P places */
#define RS_MAX_PSI (RS_MAX_PARITY + 1)   /* the coefficients of the errata locator, degree e + f <= P */

/* P of a mode: 16, 32, or 0 without a parity flag */
RS_OPS_FN unsigned rs_parity(unsigned fec) { return (fec & RS_FLAG_16) ? 16u : (fec & RS_FLAG_32) ? 32u : 0u; }

/* the 20 valid modes: none or one of the six coded modes, with none or one of
 * the two parity flags; 0 is no mode */
RS_OPS_FN int rs_mode_valid(unsigned fec)
{
    const unsigned par = fec & (RS_FLAG_16 | RS_FLAG_32), base = fec & ~(RS_FLAG_16 | RS_FLAG_32);
    if (par == (RS_FLAG_16 | RS_FLAG_32)) return 0;
    if (base == 0u) return par != 0u;
    return fec_mode_valid(base);
}

/* the convolutional part of a valid mode: 0 or one of the six coded modes */
RS_OPS_FN unsigned rs_mode_conv(unsigned fec) { return fec & ~(RS_FLAG_16 | RS_FLAG_32); }

/* ---- the erasure level and mask (include/demod.h "erasure decoding") ---------
 *
 *  level   DEMOD_FEC_ERASE(level): bits 16 .. 22 of `fec`, 0 for none; only with a parity flag and low nibble 0
 *  mask    one bit per row byte: row r has Wm = ceil(row_bytes / 64) words, byte b is bit b & 63 of word b >> 6
 */
#define RS_ERASE_SHIFT 16
#define RS_ERASE_FIELD (0x7Fu << RS_ERASE_SHIFT)

RS_OPS_FN unsigned rs_erase_level(unsigned fec) { return (fec & RS_ERASE_FIELD) >> RS_ERASE_SHIFT; }

/* the mode without the level: what goes on the air, and what every other entry takes */
RS_OPS_FN unsigned rs_erase_strip(unsigned fec) { return fec & ~RS_ERASE_FIELD; }

/* a valid mode, with or without a level; a level only with a parity flag and no convolutional code */
RS_OPS_FN int rs_erase_mode_valid(unsigned fec)
{
    const unsigned base = rs_erase_strip(fec);
    if (!rs_mode_valid(base)) return 0;
    return rs_erase_level(fec) == 0u || (rs_parity(base) != 0u && rs_mode_conv(base) == 0u);
}

/* Wm of rows of row_bytes bytes */
RS_OPS_FN unsigned rs_mask_words(unsigned row_bytes) { return (row_bytes + 63u) / 64u; }

/* byte b of a row in the row's mask words */
RS_OPS_FN int rs_mask_bit(const uint64_t *words, unsigned b) { return (int)((words[b >> 6] >> (b & 63u)) & 1u); }

/* ---- the field ------------------------------------------------------------ */

/* a alpha */
RS_OPS_FN unsigned rs_xtime(unsigned a) { return ((a << 1) ^ ((a & 0x80u) ? 0x11Du : 0u)) & 0xFFu; }

/* a b by shift and add: no table */
RS_OPS_FN unsigned rs_mul(unsigned a, unsigned b)
{
    unsigned r = 0;
    for (int i = 7; i >= 0; --i) r = rs_xtime(r) ^ (((b >> i) & 1u) ? a : 0u);
    return r;
}

/* exp[e] = alpha^e for e < 510 (so that two logarithms add without a
 * reduction), log[alpha^e] = e for e < 255; log[0] is not meaningful */
#define RS_EXP_SIZE 510
RS_OPS_FN void rs_table_entry(unsigned e, unsigned v, uint8_t *exp, uint8_t *log)
{
    exp[e] = (uint8_t)v;
    exp[e + 255u] = (uint8_t)v;
    log[v] = (uint8_t)e;
}

RS_OPS_FN unsigned rs_tmul(const uint8_t *exp, const uint8_t *log, unsigned a, unsigned b)
{
    return (a && b) ? exp[(unsigned)log[a] + log[b]] : 0u;
}

/* a / b, b != 0 */
RS_OPS_FN unsigned rs_tdiv(const uint8_t *exp, const uint8_t *log, unsigned a, unsigned b)
{
    return a ? exp[(unsigned)log[a] + 255u - log[b]] : 0u;
}

/* a alpha^z, z < 255 */
RS_OPS_FN unsigned rs_tscale(const uint8_t *exp, const uint8_t *log, unsigned a, unsigned z)
{
    return a ? exp[(unsigned)log[a] + z] : 0u;
}

#ifdef __HIPCC__
/* times a as a GF(2)-linear map held in eight registers: col[b] = a alpha^b, so that a f is the XOR of the
 * col[b] with bit b of f set (device code: the syndromes of frames_rs.hip, the parity of frames_tx.hip) */
static __device__ __forceinline__ void rs_times_cols(unsigned (&col)[8], unsigned a)
{
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        col[b] = a;
        a = rs_xtime(a);
    }
}
#endif

/* ---- the layout ------------------------------------------------------------ */

/* D: the codewords of a frame of n >= 1 bytes */
RS_OPS_FN unsigned rs_codewords(unsigned n, unsigned P) { return P ? (n + (254u - P)) / (255u - P) : 0u; }

/* k_j: the message bytes of codeword j < D */
RS_OPS_FN unsigned rs_message_bytes(unsigned n, unsigned D, unsigned j) { return (n - j + D - 1u) / D; }

/* n': the protected frame's bytes (n itself without parity) */
RS_OPS_FN unsigned rs_frame_bytes(unsigned n, unsigned P) { return n + rs_codewords(n, P) * P; }

/* where symbol x < k_j + P of codeword j sits in the frame: message byte x, or
 * parity byte x - k_j */
RS_OPS_FN unsigned rs_symbol_offset(unsigned n, unsigned D, unsigned kj, unsigned j, unsigned x)
{
    return x < kj ? j + x * D : n + (x - kj) * D + j;
}

/* symbol x of codeword j is flagged: its row byte's bit of the row's mask */
RS_OPS_FN int rs_symbol_flagged(const uint64_t *words, unsigned n, unsigned D, unsigned kj, unsigned j, unsigned x)
{
    return rs_mask_bit(words, rs_symbol_offset(n, D, kj, j, x));
}

/* ---- the encoder ----------------------------------------------------------- */

/* g(x) of P roots alpha^0 .. alpha^(P-1) into g[0 .. P], g[0] = 1 the highest coefficient */
RS_OPS_FN void rs_generator(unsigned P, uint8_t *g)
{
    unsigned root = 1;
    g[0] = 1;
    for (unsigned i = 1; i <= P; ++i) g[i] = 0;
    for (unsigned i = 0; i < P; ++i, root = rs_xtime(root))   /* times (x - alpha^i) */
        for (unsigned d = i + 1; d > 0; --d) g[d] ^= (uint8_t)rs_mul(g[d - 1], root);
}

/* the remainder of m(x) x^P by g into par[0 .. P), highest degree first; the
 * message is m[0], m[stride], .., k bytes */
RS_OPS_FN void rs_remainder(const uint8_t *m, unsigned k, unsigned stride, unsigned P, const uint8_t *g,
                            uint8_t *par)
{
    for (unsigned d = 0; d < P; ++d) par[d] = 0;
    for (unsigned i = 0; i < k; ++i) {
        const unsigned f = (unsigned)m[i * stride] ^ par[0];
        for (unsigned d = 0; d + 1 < P; ++d) par[d] = par[d + 1] ^ (uint8_t)rs_mul(f, g[d + 1]);
        par[P - 1] = (uint8_t)rs_mul(f, g[P]);
    }
}

/* the D P parity bytes frame[n .. n') of the frame's n bytes; nothing without parity */
RS_OPS_FN void rs_frame_protect(uint8_t *frame, unsigned n, unsigned P)
{
    if (!P) return;
    const unsigned D = rs_codewords(n, P);
    uint8_t g[RS_MAX_PARITY + 1], par[RS_MAX_PARITY];
    rs_generator(P, g);
    for (unsigned j = 0; j < D; ++j) {
        rs_remainder(frame + j, rs_message_bytes(n, D, j), D, P, g, par);
        for (unsigned i = 0; i < P; ++i) frame[n + i * D + j] = par[i];
    }
}

/* The greatest len with n'(h + len + c) <= W (n' increases strictly with its
 * argument), or -1 when W < n'(h + c). W < 2^31. */
RS_OPS_FN long long rs_max_len(unsigned W, unsigned h, unsigned c, unsigned P)
{
    if (rs_frame_bytes(h + c, P) > W) return -1;
    unsigned lo = h + c, hi = W;   /* n'(lo) <= W; n'(hi + 1) > W */
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo + 1u) / 2u;
        if (rs_frame_bytes(mid, P) <= W) lo = mid;
        else hi = mid - 1u;
    }
    return (long long)lo - (long long)(h + c);
}

#endif
