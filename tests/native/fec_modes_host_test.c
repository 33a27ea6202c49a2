/*
 * fec_modes_host_test.c — the coded modes' host side (csrc/demod_fec.c,
 * csrc/fec_map.h, csrc/demod_tx_frame.c) under AddressSanitizer + UBSan, on
 * exact-size heap buffers: in each of the six modes the map is a bijection
 * between the kept mother bits and [0, Nt); the encoder's air bits as +-127
 * soft values decode to the checked frame from a row of exactly the frame's
 * symbols and from the longest row of that max_len; with 4 inverted values the
 * decoder still stays inside its buffers; one frame's symbols on the host fill
 * exactly A(len) bytes; and every refusal.
 * Built and run by tests/test_fec_modes_cpu.py; no device, no Python.
 *
 *   fec_modes_host_test [seed]     prints "fec_modes_host_test OK" and exits 0
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

static const int kModes[6] = {0x01, 0x11, 0x21, 0x41, 0x51, 0x61};
static const int kBad[5] = {0, 2, 0x10, 0x31, 0x81};

/* Nt(T) by counting the kept bits */
static size_t kept_bits(int fec, size_t T)
{
    size_t n = 0;
    for (size_t m = 0; m < 2 * T; ++m) n += demod_fec_air_index(fec, m) >= 0;
    return n;
}

static void map_case(int fec, size_t T)
{
    const size_t Nt = kept_bits(fec, T), Na = (fec & DEMOD_FEC_INTERLEAVE) ? (Nt + 255) / 256 * 256 : Nt;
    uint8_t *seen = calloc(Na ? Na : 1, 1);
    for (size_t m = 0; m < 2 * T; ++m) {
        const long long a = demod_fec_air_index(fec, m);
        if (a < 0) continue;
        CHECK((size_t)a < Na && !seen[a]);
        seen[a] = 1;
    }
    if (!(fec & DEMOD_FEC_INTERLEAVE))
        for (size_t a = 0; a < Nt; ++a) CHECK(seen[a]);
    free(seen);
}

/* a frame of len data bytes, decoded from a row of n_soft values (0: exactly the frame's) */
static void frame_case(int fec, size_t len, int h, int crc, size_t extra, int flips)
{
    const size_t c = crc == DEMOD_CRC16_CCITT_FALSE ? 2 : 4, n = h + len + c;
    uint8_t *data = malloc(len ? len : 1);
    for (size_t i = 0; i < len; ++i) data[i] = (uint8_t)rnd();
    const long long Na = demod_fec_frame_symbols(len, h, crc, 1, fec);
    CHECK(Na > 0 && demod_fec_frame_symbols(len, h, crc, 3, fec) == (Na + 2) / 3);
    const size_t nb = (size_t)(Na + 7) / 8;
    uint8_t *air = malloc(nb);
    CHECK(demod_fec_frame_encode(data, len, h, crc, fec, air, nb - 1) == DEMOD_BUFFER_TOO_SMALL);
    CHECK(demod_fec_frame_encode(data, len, h, crc, fec, air, nb) == (int)nb);
    uint8_t *frame = malloc(n);
    CHECK(demod_checked_frame_encode(data, len, h, crc, frame, n) == (int)n);
    const size_t n_soft = (size_t)Na + extra;
    int8_t *soft = malloc(n_soft);
    for (size_t a = 0; a < n_soft; ++a)
        soft[a] = a < (size_t)Na ? (((air[a >> 3] >> (7 - (a & 7))) & 1) ? -127 : 127)
                                 : (int8_t)((int)(rnd() % 255) - 127);
    for (int f = 0; f < flips; ++f) {
        const size_t at = rnd() % (size_t)Na;
        soft[at] = (int8_t)-soft[at];
    }
    const long long Bd = demod_fec_row_bytes(n_soft, 1, h, fec);
    CHECK(Bd >= (long long)n);
    uint8_t *row = malloc((size_t)Bd);
    memset(row, 0xA5, (size_t)Bd);
    demod_frame_decode_t dec;
    const int rc = demod_fec_frame_decode(soft, n_soft, h, crc, fec, row, (size_t)Bd, &dec);
    CHECK(rc >= h && rc <= Bd);
    if (!flips) {
        CHECK(rc == (int)n && dec.status == DEMOD_DECODE_OK && dec.length == len);
        CHECK(dec.steps == (uint32_t)demod_coded_frame_steps(len, h, crc) && memcmp(row, frame, n) == 0);
    }
    for (size_t b = (size_t)rc; b < (size_t)Bd; ++b) CHECK(row[b] == 0xA5);
    CHECK(demod_fec_frame_decode(soft, n_soft, h, crc, fec, row, (size_t)Bd - 1, &dec) == DEMOD_BUFFER_TOO_SMALL);
    free(row);
    free(soft);
    free(frame);
    free(air);
    free(data);
}

static void tx_case(int fec, uint32_t k, size_t len)
{
    demod_tx_cfg_t x;
    memset(&x, 0, sizeof(x));
    x.sync_len = 5;
    for (int i = 0; i < 5; ++i) x.sync[i] = (uint8_t)(i % k);
    x.len_bytes = 1;
    x.crc = DEMOD_CRC16_CCITT_FALSE;
    x.fec = (uint32_t)fec;
    x.max_len = 255;
    const long long A = demod_tx_frame_symbol_count(&x, k, len);
    CHECK(A == 5 + demod_fec_frame_symbols(len, 1, DEMOD_CRC16_CCITT_FALSE, demod_bits_per_symbol(k), fec));
    uint8_t *data = malloc(len ? len : 1), *sym = malloc((size_t)A);
    for (size_t i = 0; i < len; ++i) data[i] = (uint8_t)rnd();
    CHECK(demod_tx_frame_symbols(&x, k, data, len, sym, (size_t)A - 1) == DEMOD_BUFFER_TOO_SMALL);
    CHECK(demod_tx_frame_symbols(&x, k, data, len, sym, (size_t)A) == A);
    for (long long j = 0; j < A; ++j) CHECK(sym[j] < k);
    free(sym);
    free(data);
}

static void refusals(void)
{
    int8_t soft[512];
    uint8_t row[64], out[128];
    demod_frame_decode_t dec;
    memset(soft, 0, sizeof(soft));
    for (int i = 0; i < 5; ++i) {
        const int fec = kBad[i];
        CHECK(demod_fec_air_index(fec, 0) == DEMOD_BAD_ARG);
        CHECK(demod_fec_frame_symbols(0, 1, 1, 1, fec) == DEMOD_BAD_ARG);
        CHECK(demod_fec_frame_encode(NULL, 0, 1, 1, fec, out, sizeof(out)) == DEMOD_BAD_ARG);
        CHECK(demod_fec_row_bytes(512, 1, 1, fec) == DEMOD_BAD_ARG);
        CHECK(demod_fec_frame_decode(soft, 512, 1, 1, fec, row, sizeof(row), &dec) == DEMOD_BAD_ARG);
        demod_tx_cfg_t x;
        memset(&x, 0, sizeof(x));
        x.sync_len = 1;
        x.len_bytes = 1;
        x.crc = 1;
        x.fec = (uint32_t)fec;
        x.max_len = 8;
        if (fec) CHECK(demod_tx_frame_symbol_count(&x, 2, 0) == DEMOD_BAD_ARG);
    }
    {   /* an interleaved mode with K = 3: no tone for every coded bit */
        demod_tx_cfg_t x;
        memset(&x, 0, sizeof(x));
        x.sync_len = 1;
        x.len_bytes = 1;
        x.crc = 1;
        x.fec = 0x41;
        x.max_len = 8;
        CHECK(demod_tx_frame_symbol_count(&x, 3, 0) == DEMOD_BAD_ARG);
        CHECK(demod_tx_frame_symbol_count(&x, 4, 0) == 1 + 128);   /* 2 x 72 bits -> one block, 2 bits a symbol */
    }
    /* an interleaved row shorter than one block, and the minimal one: N = 86 at 3 bits */
    CHECK(demod_fec_row_bytes(85, 3, 1, 0x41) == DEMOD_BAD_ARG && demod_fec_row_bytes(86, 3, 1, 0x41) == 15);
    CHECK(demod_fec_frame_decode(soft, 255, 1, 1, 0x41, row, sizeof(row), &dec) == DEMOD_BAD_ARG);
    CHECK(demod_fec_frame_decode(soft, 256, 1, 1, 0x41, row, sizeof(row), &dec) == 3);
    CHECK(demod_fec_frame_decode(soft, 256, 2, 1, 0x61, row, sizeof(row), &dec) == 4);    /* St 192 */
    CHECK(demod_fec_frame_decode(NULL, 256, 1, 1, 0x41, row, sizeof(row), &dec) == DEMOD_BAD_ARG);
    CHECK(demod_fec_frame_decode(soft, 256, 1, 1, 0x41, NULL, sizeof(row), &dec) == DEMOD_BAD_ARG);
    CHECK(demod_fec_frame_decode(soft, 256, 1, 1, 0x41, row, sizeof(row), NULL) == DEMOD_BAD_ARG);
    CHECK(demod_fec_frame_decode(soft, 256, 3, 1, 0x41, row, sizeof(row), &dec) == DEMOD_BAD_ARG);
    CHECK(demod_fec_frame_decode(soft, 256, 1, 0, 0x41, row, sizeof(row), &dec) == DEMOD_BAD_ARG);
    CHECK(demod_fec_air_index(0x11, (size_t)1 << 31) == DEMOD_BAD_ARG);
    /* the old functions are the new ones at fec == 1 */
    CHECK(demod_coded_frame_symbols(9, 2, 1, 3) == demod_fec_frame_symbols(9, 2, 1, 3, 1));
    CHECK(demod_coded_row_bytes(200, 3, 2) == demod_fec_row_bytes(200, 3, 2, 1));
}

int main(int argc, char **argv)
{
    if (argc > 1) g_rng ^= (uint64_t)strtoull(argv[1], NULL, 0);
    refusals();
    for (int i = 0; i < 6; ++i) {
        const int fec = kModes[i];
        for (size_t T = 0; T < 200; T += 1 + T / 7) map_case(fec, T);
        for (int h = 1; h <= 2; ++h)
            for (int crc = 1; crc <= 2; ++crc) {
                const size_t lens[] = {0, 1, 5, 6, 24, 38, 61};
                for (size_t j = 0; j < sizeof(lens) / sizeof(lens[0]); ++j) {
                    frame_case(fec, lens[j], h, crc, 0, 0);
                    frame_case(fec, lens[j], h, crc, 1 + rnd() % 300, 0);
                    frame_case(fec, lens[j], h, crc, rnd() % 300, 4);
                }
            }
        for (uint32_t k = 2; k <= 16; k *= 2) {
            tx_case(fec, k, 0);
            tx_case(fec, k, 38);
            tx_case(fec, k, 255);
        }
    }
    printf("fec_modes_host_test OK\n");
    return 0;
}
