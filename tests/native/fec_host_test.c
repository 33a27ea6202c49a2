/*
 * fec_host_test.c — the host side of the coded frame (csrc/demod_fec.c) under
 * AddressSanitizer + UBSan, on exact-size heap buffers: the encoder's coded
 * bits as +-127 soft values with 4 of them inverted and random values behind
 * the frame must decode to the checked frame, at the edge lengths (0, 1, either
 * side of 8 n + 6 = 8 h + 64, max_len), a header above max_len, a header of all
 * ones, all-zero soft values, an odd C and the minimal row; and every refusal.
 * Built and run by tests/test_frames_fec_cpu.py; no device, no Python.
 *
 *   fec_host_test [cases] [seed]     prints "fec_host_test OK" and exits 0
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/demod.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

/* One row of n_soft values holding a coded frame of len data bytes with `flips`
 * inverted values; decoded and compared with the checked frame. */
static void frame_case(size_t len, int h, int crc, size_t n_soft, int flips)
{
    const size_t c = crc == DEMOD_CRC16_CCITT_FALSE ? 2 : 4;
    uint8_t *data = malloc(len ? len : 1);
    for (size_t i = 0; i < len; ++i) data[i] = (uint8_t)rnd();
    const long long T = demod_coded_frame_steps(len, h, crc);
    CHECK(T > 0 && demod_coded_frame_symbols(len, h, crc, 1) == 2 * T);
    const size_t nb = (size_t)(2 * T + 7) / 8;
    uint8_t *coded = malloc(nb);
    CHECK(demod_coded_frame_encode(data, len, h, crc, coded, nb - 1) == DEMOD_BUFFER_TOO_SMALL);
    CHECK(demod_coded_frame_encode(data, len, h, crc, coded, nb) == (int)nb);
    uint8_t *frame = malloc(h + len + c);
    CHECK(demod_checked_frame_encode(data, len, h, crc, frame, h + len + c) == (int)(h + len + c));
    int8_t *soft = malloc(n_soft);
    for (size_t m = 0; m < n_soft; ++m) {
        if (m < (size_t)(2 * T))
            soft[m] = ((coded[m >> 3] >> (7 - (m & 7))) & 1) ? -127 : 127;
        else
            soft[m] = (int8_t)((int)(rnd() % 255) - 127);
    }
    const size_t span = (size_t)(2 * T) < n_soft ? (size_t)(2 * T) : n_soft;
    for (int f = 0; f < flips; ++f) {
        size_t at = rnd() % span;
        while (soft[at] != 127 && soft[at] != -127) at = rnd() % span;
        soft[at] = (int8_t)(soft[at] > 0 ? -126 : 126);    /* inverted, and not picked again */
    }
    const size_t St = n_soft / 2, Bd = (St - 6) / 8, max_len = Bd - h - c;
    uint8_t *row = malloc(Bd);
    memset(row, 0xA5, Bd);
    demod_frame_decode_t dec;
    const int rc = demod_coded_frame_decode(soft, n_soft, h, crc, row, Bd, &dec);
    if (len <= max_len) {
        CHECK(rc == (int)(h + len + c) && dec.status == DEMOD_DECODE_OK && dec.length == len);
        CHECK(dec.steps == (uint32_t)T && memcmp(row, frame, h + len + c) == 0);
        CHECK(dec.metric == 127 * 2 * (int)T - (127 + 126) * flips);
    } else {
        CHECK(rc == h && dec.status == DEMOD_DECODE_BAD_LENGTH && dec.length == len);
        CHECK(dec.metric == 0 && dec.steps == 0 && memcmp(row, frame, h) == 0);
    }
    for (size_t b = (size_t)rc; b < Bd; ++b) CHECK(row[b] == 0xA5);
    if (Bd > 0) CHECK(demod_coded_frame_decode(soft, n_soft, h, crc, row, Bd - 1, &dec) == DEMOD_BUFFER_TOO_SMALL);
    free(row);
    free(soft);
    free(frame);
    free(coded);
    free(data);
}

static void edges(int h, int crc)
{
    const size_t c = crc == DEMOD_CRC16_CCITT_FALSE ? 2 : 4;
    const size_t t0 = 8 * (size_t)h + DEMOD_FEC_DEPTH;
    /* the minimal row, one value more (odd C), and rows of max_len 24 and 25 values more */
    const size_t shapes[] = {2 * t0, 2 * t0 + 1, 2 * (8 * (h + 24 + c) + 6), 2 * (8 * (h + 24 + c) + 6) + 25};
    for (size_t s = 0; s < sizeof(shapes) / sizeof(shapes[0]); ++s) {
        const size_t n_soft = shapes[s], Bd = (n_soft / 2 - 6) / 8, max_len = Bd - h - c;
        const size_t lens[] = {0, 1, 7 - c, 8 - c, max_len, max_len + 1};
        for (size_t i = 0; i < sizeof(lens) / sizeof(lens[0]); ++i)
            if (lens[i] <= max_len + 1) frame_case(lens[i], h, crc, n_soft, lens[i] <= max_len ? 4 : 0);
        /* all-zero soft values: every comparison ties, the all-zero path wins: len 0 and a zero CRC field */
        int8_t *soft = calloc(n_soft, 1);
        uint8_t *row = malloc(Bd);
        demod_frame_decode_t dec;
        CHECK(demod_coded_frame_decode(soft, n_soft, h, crc, row, Bd, &dec) == (int)(h + c));
        CHECK(dec.length == 0 && dec.metric == 0 && dec.status == DEMOD_DECODE_OK && dec.steps == t0);
        for (size_t b = 0; b < h + c; ++b) CHECK(row[b] == 0);
        /* a header of all ones */
        for (size_t m = 0; m < n_soft; ++m) soft[m] = (int8_t)((int)(rnd() % 255) - 127);
        {   /* no frame has this header: the encoder's recurrence, restated */
            unsigned reg = 0;
            for (size_t t = 0; t < t0; ++t) {
                const unsigned u = t < 8 * (size_t)h ? 1u : 0u;
                reg = ((reg << 1) | u) & 0x7Fu;
                soft[2 * t] = __builtin_parity(reg & 0171u) ? -127 : 127;
                soft[2 * t + 1] = __builtin_parity(reg & 0133u) ? -127 : 127;
            }
        }
        memset(row, 0xA5, Bd);
        CHECK(demod_coded_frame_decode(soft, n_soft, h, crc, row, Bd, &dec) == h);
        CHECK(dec.status == DEMOD_DECODE_BAD_LENGTH && dec.length == (h == 1 ? 0xFFu : 0xFFFFu));
        for (size_t b = 0; b < Bd; ++b) CHECK(row[b] == (b < (size_t)h ? 0xFF : 0xA5));
        free(row);
        free(soft);
    }
}

static void refusals(void)
{
    int8_t soft[200];
    uint8_t row[16], out[64];
    demod_frame_decode_t dec;
    memset(soft, 0, sizeof(soft));
    CHECK(demod_coded_frame_decode(NULL, 200, 1, 1, row, 16, &dec) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_decode(soft, 200, 1, 1, NULL, 16, &dec) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_decode(soft, 200, 1, 1, row, 16, NULL) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_decode(soft, 200, 0, 1, row, 16, &dec) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_decode(soft, 200, 3, 1, row, 16, &dec) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_decode(soft, 200, 1, 0, row, 16, &dec) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_decode(soft, 200, 1, 3, row, 16, &dec) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_decode(soft, 143, 1, 1, row, 16, &dec) == DEMOD_BAD_ARG);   /* St 71 */
    CHECK(demod_coded_frame_decode(soft, 159, 2, 1, row, 16, &dec) == DEMOD_BAD_ARG);   /* St 79 */
    CHECK(demod_coded_frame_decode(soft, 2 * (8 * 4100 + 6), 1, 1, row, 16, &dec) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_decode(soft, 144, 1, 1, row, 16, &dec) == 3);
    CHECK(demod_coded_frame_encode(NULL, 1, 1, 1, out, 64) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_encode(NULL, 0, 1, 1, NULL, 64) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_encode(NULL, 0, 1, 1, out, 64) == 18);      /* 2 x 72 bits */
    CHECK(demod_coded_frame_encode(NULL, 0, 1, 1, out, 17) == DEMOD_BUFFER_TOO_SMALL);
    CHECK(demod_coded_frame_encode(NULL, 0, 0, 1, out, 64) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_encode(NULL, 0, 1, 0, out, 64) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_steps(256, 1, 1) == DEMOD_FRAME_TOO_LARGE);
    CHECK(demod_coded_frame_steps(4097, 2, 2) == DEMOD_FRAME_TOO_LARGE);
    CHECK(demod_coded_frame_steps(4096, 2, 2) == 8 * 4102 + 6);
    CHECK(demod_coded_frame_steps(0, 2, 1) == 80 && demod_coded_frame_steps(5, 1, 1) == 72);
    CHECK(demod_coded_frame_steps(6, 1, 1) == 78);
    CHECK(demod_coded_frame_symbols(0, 1, 1, 3) == 48 && demod_coded_frame_symbols(0, 1, 1, 0) == DEMOD_BAD_ARG);
    CHECK(demod_coded_frame_symbols(0, 1, 1, 5) == DEMOD_BAD_ARG);
    CHECK(demod_coded_row_bytes(144, 1, 1) == 8 && demod_coded_row_bytes(143, 1, 1) == DEMOD_BAD_ARG);
    CHECK(demod_coded_row_bytes(48, 3, 1) == 8 && demod_coded_row_bytes(49, 3, 1) == 8);
    CHECK(demod_coded_row_bytes(144, 0, 1) == DEMOD_BAD_ARG && demod_coded_row_bytes(144, 1, 3) == DEMOD_BAD_ARG);
    float p[16];
    int8_t q[4];
    for (int i = 0; i < 16; ++i) p[i] = (float)(i + 1);
    CHECK(demod_soft_bits(NULL, 2, q) == DEMOD_BAD_ARG && demod_soft_bits(p, 2, NULL) == DEMOD_BAD_ARG);
    CHECK(demod_soft_bits(p, 1, q) == DEMOD_BAD_ARG && demod_soft_bits(p, 3, q) == DEMOD_BAD_ARG);
    CHECK(demod_soft_bits(p, 32, q) == DEMOD_BAD_ARG && demod_soft_bits(p, 0, q) == DEMOD_BAD_ARG);
    CHECK(demod_soft_bits(p, 2, q) == 1 && q[0] == -42);                /* rint(127 (1 - 2) / 3) */
    CHECK(demod_soft_bits(p, 16, q) == 4 && q[0] == -42 && q[3] == -4); /* 8 v 16, 15 v 16 */
}

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? atoi(argv[1]) : 200;
    if (argc > 2) g_rng ^= (uint64_t)strtoull(argv[2], NULL, 0);
    refusals();
    for (int h = 1; h <= 2; ++h)
        for (int crc = 1; crc <= 2; ++crc) edges(h, crc);
    for (int i = 0; i < cases; ++i) {
        const int h = 1 + (int)(rnd() & 1), crc = 1 + (int)(rnd() & 1);
        const size_t c = crc == 1 ? 2 : 4, len = rnd() % 41;
        const size_t T = 8 * (h + len + c) + 6 > 8 * (size_t)h + 64 ? 8 * (h + len + c) + 6 : 8 * (size_t)h + 64;
        frame_case(len, h, crc, 2 * T + rnd() % 300, 4);
    }
    printf("fec_host_test OK\n");
    return 0;
}
