/*
 * demod_frame_check.c — the transmit side of the checked frame (include/demod.h
 * "checked frames", DESIGN.md §4.9 "Checked frames"): the two CRCs and
 *
 *   len (h bytes, big-endian) || data (len bytes) || CRC (c bytes, big-endian)
 *
 * with the CRC over the length field and the data. Both kinds are
 * non-reflected with xorout 0 and differ in width alone; the register is kept
 * in the top `width` bits of a 32-bit word, so one loop serves both (the
 * device restates it the same way, frames_check.hip). Pure host byte work.
 */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/demod.h"

/* width, or 0 for an unknown kind; *poly and *init top-aligned in 32 bits */
static int crc_kind(int crc, uint32_t *poly, uint32_t *init)
{
    if (crc == DEMOD_CRC16_CCITT_FALSE) {
        *poly = 0x1021u << 16;
        *init = 0xFFFFu << 16;
        return 16;
    }
    if (crc == DEMOD_CRC32_MPEG2) {
        *poly = 0x04C11DB7u;
        *init = 0xFFFFFFFFu;
        return 32;
    }
    return 0;
}

uint32_t demod_crc(int crc, const uint8_t *data, size_t len)
{
    uint32_t poly, reg;
    const int width = crc_kind(crc, &poly, &reg);
    if (width == 0 || (!data && len)) return 0;
    for (size_t i = 0; i < len; ++i) {
        reg ^= (uint32_t)data[i] << 24;
        for (int b = 0; b < 8; ++b) reg = (reg << 1) ^ ((reg >> 31) ? poly : 0u);
    }
    return reg >> (32 - width);
}

long long demod_checked_frame_size(size_t len, int len_bytes, int crc)
{
    uint32_t poly, init;
    const int width = crc_kind(crc, &poly, &init);
    if (width == 0 || (len_bytes != 1 && len_bytes != 2)) return DEMOD_BAD_ARG;
    if (len > DEMOD_MAX_FRAME_PAYLOAD || len > (len_bytes == 1 ? 0xFFu : 0xFFFFu))
        return DEMOD_FRAME_TOO_LARGE;
    return (long long)(len_bytes + len + width / 8);
}

int demod_checked_frame_encode(const uint8_t *data, size_t len, int len_bytes, int crc, uint8_t *out,
                               size_t cap)
{
    const long long need = demod_checked_frame_size(len, len_bytes, crc);
    if (need < 0) return (int)need;
    if ((!data && len) || !out) return DEMOD_BAD_ARG;
    if ((size_t)need > cap) return DEMOD_BUFFER_TOO_SMALL;
    size_t p = 0;
    if (len_bytes == 2) out[p++] = (uint8_t)(len >> 8);
    out[p++] = (uint8_t)len;
    if (len) memcpy(out + p, data, len);
    p += len;
    const uint32_t v = demod_crc(crc, out, p);
    for (int c = (int)((size_t)need - p) - 1; c >= 0; --c) out[p++] = (uint8_t)(v >> (8 * c));
    return (int)p;
}
