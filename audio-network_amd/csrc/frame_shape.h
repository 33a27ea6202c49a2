/*
 * frame_shape.h — the one copy of a frame row's shape (include/demod.h "checked frames", "coded frames",
 * "Reed-Solomon outer code"): what the `fec` mode, the CRC kind and len_bytes make of frame_symbols, and a
 * frame's span on the air. Shared by the host entry points of the stages over a scan's rows, the host C
 * (demod_fec.c, demod_rs.c, demod_tx_frame.c) and the stages' kernels (frame_rows.h, frames_tx.hip). Plain
 * integer code that compiles for all of them.
 *
 *  row    N symbols of `bits` bits are C = N bits air bits: B = ceil(C / 8) packed bytes, or with the
 *         convolutional code St trellis steps that decode to Bd = (St - 6) / 8 bytes
 *  frame  len (h bytes) || data || CRC (c bytes), n bytes; with an outer code of P parity bytes n' (rs_ops.h)
 *  level  DEMOD_FEC_ERASE(level) changes none of this: the entries that take it (demod_frames_coded, the receiver)
 *         strip it (rs_ops.h rs_erase_strip) before they ask for a shape, and frame_shape_fill refuses it like any
 *         unknown bit; a row's mask has rs_mask_words(row_bytes) words
 */
#ifndef FSKD_FRAME_SHAPE_H
#define FSKD_FRAME_SHAPE_H

#include "../../include/demod.h"
#include "rs_ops.h"

#define FRAME_SHAPE_FN FEC_MAP_FN

/* c: the CRC's bytes, or 0 for an unknown kind */
FRAME_SHAPE_FN int frame_crc_bytes(int crc)
{
    return crc == DEMOD_CRC16_CCITT_FALSE ? 2 : crc == DEMOD_CRC32_MPEG2 ? 4 : 0;
}

/* St of a row of C air bits in one of the six coded modes (fec_map.h): the greatest T with Nt(T) <= Cu.
 * A mapped mode's C beyond 2^32 - 1: 0. */
FRAME_SHAPE_FN unsigned long long frame_row_steps(unsigned conv, unsigned long long C)
{
    if (!fec_mode_mapped(conv)) return C / 2;
    return C > 0xFFFFFFFFu ? 0 : fec_steps_within(conv, fec_usable_bits(conv, (unsigned)C));
}

/* max_len: the greatest len whose frame (its n bytes, or with an outer code its n') fits a row of W < 2^31
 * bytes. Negative where none fits; the stages refuse that and more than DEMOD_MAX_FRAME_PAYLOAD. */
FRAME_SHAPE_FN long long frame_max_len(unsigned W, unsigned h, unsigned c, unsigned P)
{
    return P ? rs_max_len(W, h, c, P) : (long long)W - (long long)(h + c);
}

/* A frame's span on the air, the one copy: the symbols of `bits` bits that a frame of len data bytes occupies
 * behind its word. Its n' bytes' bits; with the convolutional code `conv` its T = max(8 n' + 6, 8 h +
 * DEMOD_FEC_DEPTH) steps, *kept = Nt(T) code bits and Na air bits (T and Nt 0 without the code). Arithmetic on
 * accepted values alone: len <= DEMOD_MAX_FRAME_PAYLOAD, h, c, bits and the mode valid; the callers refuse
 * the rest. */
FRAME_SHAPE_FN unsigned frame_air_symbols(unsigned len, unsigned h, unsigned c, unsigned bits, unsigned conv,
                                          unsigned P, unsigned *steps, unsigned *kept)
{
    unsigned span = 8u * rs_frame_bytes(h + len + c, P);
    *steps = *kept = 0;
    if (conv) {
        const unsigned least = 8u * h + DEMOD_FEC_DEPTH;
        *steps = span + 6u > least ? span + 6u : least;
        *kept = fec_kept_bits(conv, *steps);
        span = fec_air_bits(conv, *kept);
    }
    return (span + bits - 1u) / bits;
}

/* The widest row any mode takes: n' at the payload limit with h = 2, CRC-32 and P = 32 (D = 19) */
#define FRAME_MAX_ROW_BYTES (2 + DEMOD_MAX_FRAME_PAYLOAD + 4 + 19 * RS_MAX_PARITY)

/* B of plain rows of frame_symbols symbols of `bits` bits, whatever header, CRC and parity flag they are read
 * with (the erasure masks' producer, which reads none of them); 0 for no symbol or more than the widest row. */
FRAME_SHAPE_FN unsigned frame_plain_row_bytes(int bits, size_t frame_symbols)
{
    if (frame_symbols == 0 || frame_symbols > 8u * FRAME_MAX_ROW_BYTES) return 0;
    const unsigned B = ((unsigned)frame_symbols * (unsigned)bits + 7u) / 8u;
    return B <= FRAME_MAX_ROW_BYTES ? B : 0u;
}

struct frame_shape {
    unsigned row_bytes;                 /* B, or Bd in a coded mode */
    unsigned max_len;                   /* <= DEMOD_MAX_FRAME_PAYLOAD */
    unsigned steps;                     /* St, or 0 without the convolutional code */
    int len_bytes, crc_bytes, bits;     /* h, c */
    int fec, fec_depth;                 /* the convolutional part of the mode and DEMOD_FEC_DEPTH, or both 0 */
    int parity;                         /* P of the outer code, or 0 */
};

/* The shape of rows of frame_symbols symbols of `bits` bits; fec 0: the scan's packed rows. Nonzero for what
 * every stage refuses: an invalid mode, len_bytes not 1 or 2, an unknown CRC kind, 2^31 symbols or more, a
 * coded mode with K not 2^bits, a row below the shortest coded frame's 8 h + DEMOD_FEC_DEPTH steps, no
 * max_len or one beyond DEMOD_MAX_FRAME_PAYLOAD. */
FRAME_SHAPE_FN int frame_shape_fill(struct frame_shape *s, int bits, int k_is_power_of_two, size_t frame_symbols,
                                    int len_bytes, int crc, int fec)
{
    const unsigned h = (unsigned)len_bytes, c = (unsigned)frame_crc_bytes(crc);
    if ((fec && !rs_mode_valid((unsigned)fec)) || (len_bytes != 1 && len_bytes != 2) || c == 0) return 1;
    if (frame_symbols > 0x7FFFFFFF) return 1;
    const unsigned conv = rs_mode_conv((unsigned)fec), P = rs_parity((unsigned)fec);
    const unsigned long long C = (unsigned long long)frame_symbols * (unsigned)bits;
    unsigned long long B = (C + 7) / 8, St = 0;
    if (conv) {
        St = frame_row_steps(conv, C);
        if (!k_is_power_of_two || St < 8 * h + DEMOD_FEC_DEPTH) return 1;
        B = (St - 6) / 8;
    }
    const long long M = frame_max_len((unsigned)B, h, c, P);
    if (M < 0 || M > DEMOD_MAX_FRAME_PAYLOAD) return 1;
    s->row_bytes = (unsigned)B;
    s->max_len = (unsigned)M;
    s->steps = (unsigned)St;
    s->len_bytes = len_bytes;
    s->crc_bytes = (int)c;
    s->bits = bits;
    s->fec = (int)conv;
    s->fec_depth = conv ? DEMOD_FEC_DEPTH : 0;
    s->parity = (int)P;
    return 0;
}

#endif
