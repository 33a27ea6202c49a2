/*
 * tx_host_test.c — the device-free part of the transmitter
 * (csrc/demod_tx_frame.c over demod_frame_check.c, demod_fec.c and
 * demod_frame.c) under AddressSanitizer + UBSan, on exact-size heap buffers:
 * for random formats, tone counts and lengths the frame's symbols are held
 * against the byte encoders and demod_unpack_symbols called directly, packed
 * back into the frame's bytes, and every refusal is asked for with a buffer one
 * symbol short. Built and run by tests/test_tx_cpu.py; no device, no Python.
 *
 *   tx_host_test [cases] [seed]     prints "tx_host_test OK" and exits 0
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/demod.h"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

static uint64_t g_state;
static uint32_t rnd(void)
{
    g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(g_state >> 33);
}

static void frame_case(uint32_t k, int h, int crc, int fec, size_t len, size_t max_len, size_t L)
{
    demod_tx_cfg_t x;
    memset(&x, 0, sizeof(x));
    x.sync_len = (uint32_t)L;
    for (size_t i = 0; i < L; ++i) x.sync[i] = (uint8_t)(rnd() % k);
    x.len_bytes = (uint32_t)h;
    x.crc = (uint32_t)crc;
    x.fec = (uint32_t)fec;
    x.max_len = (uint32_t)max_len;
    const int bits = demod_bits_per_symbol(k);
    const long long A = demod_tx_frame_symbol_count(&x, k, len);
    CHECK(A > (long long)L);
    const long long Sp = A - (long long)L;

    uint8_t *data = malloc(len ? len : 1);
    CHECK(data);
    for (size_t i = 0; i < len; ++i) data[i] = (uint8_t)rnd();
    uint8_t *out = malloc((size_t)A);
    CHECK(out);
    CHECK(demod_tx_frame_symbols(&x, k, data, len, out, (size_t)A) == A);
    CHECK(demod_tx_frame_symbols(&x, k, data, len, out, (size_t)A - 1) == DEMOD_BUFFER_TOO_SMALL);
    CHECK(memcmp(out, x.sync, L) == 0);
    for (long long i = 0; i < A; ++i) CHECK(out[i] < (1u << bits));

    /* the payload against the encoders called directly, one 0 byte behind their bytes */
    const size_t cap = (size_t)((Sp * bits + 7) / 8) + 1;
    uint8_t *bytes = calloc(cap, 1);
    CHECK(bytes);
    const int nb = fec ? demod_coded_frame_encode(data, len, h, crc, bytes, cap - 1)
                       : demod_checked_frame_encode(data, len, h, crc, bytes, cap - 1);
    CHECK(nb > 0 && (size_t)nb <= cap - 1);
    uint8_t *want = malloc((size_t)Sp);
    CHECK(want);
    CHECK(demod_unpack_symbols(bytes, (size_t)Sp, bits, want, (size_t)Sp) == Sp);
    CHECK(memcmp(out + L, want, (size_t)Sp) == 0);
    /* and packed back: the frame's bytes, pad bits 0 */
    uint8_t *back = malloc(cap);
    CHECK(back);
    const int pb = demod_pack_symbols(out + L, (size_t)Sp, bits, back, cap);
    CHECK(pb >= nb && memcmp(back, bytes, (size_t)nb) == 0);
    for (int i = nb; i < pb; ++i) CHECK(back[i] == 0);

    if (len + 1 > max_len) CHECK(demod_tx_frame_symbol_count(&x, k, max_len + 1) == DEMOD_FRAME_TOO_LARGE);
    free(back);
    free(want);
    free(bytes);
    free(out);
    free(data);
}

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? atoi(argv[1]) : 200;
    g_state = argc > 2 ? (uint64_t)atoll(argv[2]) : 1;
    static const uint32_t ks[] = {2, 4, 8, 16, 3, 5, 12};
    for (int i = 0; i < cases; ++i) {
        const int fec = (int)(rnd() & 1u);
        const uint32_t k = ks[rnd() % (fec ? 4 : 7)];
        const int h = 1 + (int)(rnd() & 1u);
        const int crc = (rnd() & 1u) ? DEMOD_CRC16_CCITT_FALSE : DEMOD_CRC32_MPEG2;
        const size_t most = h == 1 ? 255 : DEMOD_MAX_FRAME_PAYLOAD;
        size_t len = rnd() % 8 == 0 ? most : rnd() % 80;
        if (len > most) len = most;
        const size_t max_len = rnd() & 1u ? len : most;
        frame_case(k, h, crc, fec, len, max_len, 1 + rnd() % DEMOD_MAX_SYNC);
    }
    /* refusals */
    demod_tx_cfg_t x;
    memset(&x, 0, sizeof(x));
    x.sync_len = 4;
    x.len_bytes = 2;
    x.crc = DEMOD_CRC16_CCITT_FALSE;
    x.max_len = 16;
    uint8_t buf[512], d[16] = {0};
    CHECK(demod_tx_frame_symbol_count(NULL, 2, 0) == DEMOD_BAD_ARG);
    CHECK(demod_tx_frame_symbol_count(&x, 1, 0) == DEMOD_BAD_ARG);
    CHECK(demod_tx_frame_symbol_count(&x, 17, 0) == DEMOD_BAD_ARG);
    CHECK(demod_tx_frame_symbol_count(&x, 2, 17) == DEMOD_FRAME_TOO_LARGE);
    CHECK(demod_tx_frame_symbols(&x, 2, NULL, 1, buf, sizeof(buf)) == DEMOD_BAD_ARG);
    CHECK(demod_tx_frame_symbols(&x, 2, d, 1, NULL, sizeof(buf)) == DEMOD_BAD_ARG);
    x.sync[3] = 2;
    CHECK(demod_tx_frame_symbols(&x, 2, d, 1, buf, sizeof(buf)) == DEMOD_BAD_ARG);
    x.sync[3] = 0;
    x.fec = DEMOD_FEC_CONV_K7;
    CHECK(demod_tx_frame_symbol_count(&x, 5, 0) == DEMOD_BAD_ARG);
    x.fec = 2;
    CHECK(demod_tx_frame_symbol_count(&x, 4, 0) == DEMOD_BAD_ARG);
    x.fec = 0;
    x.crc = 3;
    CHECK(demod_tx_frame_symbol_count(&x, 4, 0) == DEMOD_BAD_ARG);
    x.crc = DEMOD_CRC32_MPEG2;
    x.len_bytes = 3;
    CHECK(demod_tx_frame_symbol_count(&x, 4, 0) == DEMOD_BAD_ARG);
    x.len_bytes = 1;
    x.max_len = 300;
    CHECK(demod_tx_frame_symbol_count(&x, 4, 256) == DEMOD_FRAME_TOO_LARGE);
    x.sync_len = 0;
    CHECK(demod_tx_frame_symbol_count(&x, 4, 0) == DEMOD_BAD_ARG);
    x.sync_len = DEMOD_MAX_SYNC + 1;
    CHECK(demod_tx_frame_symbol_count(&x, 4, 0) == DEMOD_BAD_ARG);
    printf("tx_host_test OK\n");
    return 0;
}
