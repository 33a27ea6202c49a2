/*
 * demod_tx_frame.c — the device-free part of the transmitter (include/demod.h
 * "transmitter", DESIGN.md §4.9 "Transmitter"): the symbols of one frame on
 * the air, built from the existing byte encoders. This is the reference the
 * write launch of frames_tx.hip is held to, symbol for symbol. Pure host work.
 */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "frame_shape.h"

/* bits, or a negative code for what the format or K rules out */
static int tx_format_bits(const demod_tx_cfg_t *x, uint32_t k)
{
    if (!x || k < 2 || k > DEMOD_MAX_TONES) return DEMOD_BAD_ARG;
    if (x->sync_len < 1 || x->sync_len > DEMOD_MAX_SYNC) return DEMOD_BAD_ARG;
    if (x->len_bytes != 1 && x->len_bytes != 2) return DEMOD_BAD_ARG;
    if (frame_crc_bytes((int)x->crc) == 0) return DEMOD_BAD_ARG;
    if (x->fec != 0 && !rs_mode_valid(x->fec)) return DEMOD_BAD_ARG;
    if (rs_mode_conv(x->fec) && (k & (k - 1)) != 0) return DEMOD_BAD_ARG;
    return demod_bits_per_symbol(k);
}

long long demod_tx_frame_symbol_count(const demod_tx_cfg_t *x, uint32_t k, size_t len)
{
    const int bits = tx_format_bits(x, k);
    if (bits < 0) return bits;
    if (len > x->max_len) return DEMOD_FRAME_TOO_LARGE;
    long long sp;
    if (rs_mode_conv(x->fec)) {
        sp = demod_fec_frame_symbols(len, (int)x->len_bytes, (int)x->crc, bits, (int)x->fec);
    } else {
        /* the frame's n bytes, or with an outer code its n' (frame_shape.h) */
        unsigned T, Nt;
        sp = demod_checked_frame_size(len, (int)x->len_bytes, (int)x->crc);
        if (sp >= 0)
            sp = frame_air_symbols((unsigned)len, x->len_bytes, (unsigned)frame_crc_bytes((int)x->crc), (unsigned)bits,
                                   0, rs_parity(x->fec), &T, &Nt);
    }
    return sp < 0 ? sp : (long long)x->sync_len + sp;
}

long long demod_tx_frame_symbols(const demod_tx_cfg_t *x, uint32_t k, const uint8_t *data, size_t len,
                                 uint8_t *out, size_t cap)
{
    const long long A = demod_tx_frame_symbol_count(x, k, len);
    if (A < 0) return A;
    if ((!data && len) || !out) return DEMOD_BAD_ARG;
    const size_t L = x->sync_len;
    for (size_t i = 0; i < L; ++i)
        if (x->sync[i] >= k) return DEMOD_BAD_ARG;
    if ((size_t)A > cap) return DEMOD_BUFFER_TOO_SMALL;
    const int bits = demod_bits_per_symbol(k);
    /* the frame's bytes, with a 0 byte behind them: the last symbol's missing bits */
    /* (sized by rate 1/2, the most bits, and one interleaver block of rounding) */
    /* (the frame with the outer code's most parity: 19 codewords of 32 bytes) */
    uint8_t bytes[(2 * (8 * (2 + DEMOD_MAX_FRAME_PAYLOAD + 4 + 19 * RS_MAX_PARITY) + 6) + 7) / 8 +
                  DEMOD_FEC_IL_ROWS * DEMOD_FEC_IL_COLS / 8 + 1];
    memset(bytes, 0, sizeof(bytes));
    int nb;
    if (rs_mode_conv(x->fec)) {
        nb = demod_fec_frame_encode(data, len, (int)x->len_bytes, (int)x->crc, (int)x->fec, bytes,
                                    sizeof(bytes) - 1);
    } else {
        nb = demod_checked_frame_encode(data, len, (int)x->len_bytes, (int)x->crc, bytes, sizeof(bytes) - 1);
        if (nb >= 0) rs_frame_protect(bytes, (unsigned)nb, rs_parity(x->fec));
    }
    if (nb < 0) return nb;
    memcpy(out, x->sync, L);
    const int rc = demod_unpack_symbols(bytes, (size_t)A - L, bits, out + L, cap - L);
    return rc < 0 ? rc : A;
}
