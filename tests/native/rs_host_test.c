/*
 * rs_host_test.c — the host side of the Reed-Solomon outer code (demod_rs.c,
 * and the parity modes of demod_fec.c and demod_tx_frame.c) in a program of
 * its own, built with -fsanitize=address,undefined by tests/test_rs_cpu.py:
 * the pinned vectors, every frame shape with up to t wrong bytes a codeword
 * (which must come back), t + 1 and random rows (which must not touch a byte
 * past the frame), the refusals, and one frame through the coded chain.
 *
 *   rs_host_test [seed]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/demod.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);           \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

static uint64_t rng_state;
static uint32_t rnd(void)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static void pins(void)
{
    static const uint8_t qr_msg[16] = {0x20, 0x5B, 0x0B, 0x78, 0xD1, 0x72, 0xDC, 0x4D,
                                       0x43, 0x40, 0xEC, 0x11, 0xEC, 0x11, 0xEC, 0x11};
    static const uint8_t qr_par[10] = {0xC4, 0x23, 0x27, 0x77, 0xEB, 0xD7, 0xE7, 0xE2, 0x5D, 0x17};
    static const uint8_t g16[17] = {0x01, 0x3B, 0x0D, 0x68, 0xBD, 0x44, 0xD1, 0x1E, 0x08,
                                    0xA3, 0x41, 0x29, 0xE5, 0x62, 0x32, 0x24, 0x3B};
    static const uint8_t p16[16] = {0x57, 0x55, 0xa7, 0x70, 0xf1, 0xf6, 0x9c, 0x34,
                                    0x92, 0x0d, 0x63, 0x86, 0xa4, 0x19, 0x1a, 0x96};
    static const uint8_t p32[32] = {0x4e, 0xff, 0xf5, 0x5e, 0xfc, 0x5f, 0x53, 0x51, 0x28, 0x4f, 0xef,
                                    0x58, 0x77, 0x3a, 0xaa, 0xbf, 0xda, 0x9e, 0xe0, 0x7e, 0x54, 0x4d,
                                    0xd2, 0x35, 0x87, 0xcd, 0x18, 0x9f, 0xc3, 0x38, 0xda, 0xca};
    uint8_t out[33];
    CHECK(demod_rs_encode(qr_msg, 16, 10, out) == 10 && memcmp(out, qr_par, 10) == 0);
    CHECK(demod_rs_generator(16, out) == 17 && memcmp(out, g16, 17) == 0);
    CHECK(demod_rs_encode((const uint8_t *)"123456789", 9, 16, out) == 16 && memcmp(out, p16, 16) == 0);
    CHECK(demod_rs_encode((const uint8_t *)"123456789", 9, 32, out) == 32 && memcmp(out, p32, 32) == 0);
    CHECK(demod_rs_encode(qr_msg, 16, 0, out) == DEMOD_BAD_ARG && demod_rs_encode(qr_msg, 16, 33, out) == DEMOD_BAD_ARG);
    CHECK(demod_rs_encode(qr_msg, 240, 16, out) == DEMOD_BAD_ARG && demod_rs_generator(33, out) == DEMOD_BAD_ARG);
    CHECK(demod_rs_frame_size(DEMOD_MAX_FRAME_PAYLOAD, 2, DEMOD_CRC32_MPEG2, DEMOD_FEC_RS16) == 4390);
    CHECK(demod_rs_frame_size(DEMOD_MAX_FRAME_PAYLOAD, 2, DEMOD_CRC32_MPEG2, DEMOD_FEC_RS32) == 4710);
}

/* a frame of len bytes with `wrong` wrong bytes in every codeword, in a row
 * of exactly W bytes (heap: the sanitizer sees one byte past it) */
static void one_frame(size_t len, int h, int crc, int fec, unsigned wrong, size_t pad)
{
    const unsigned P = fec & DEMOD_FEC_RS16 ? 16 : 32, t = P / 2;
    const long long np = demod_rs_frame_size(len, h, crc, fec);
    CHECK(np > 0);
    const size_t W = (size_t)np + pad;
    uint8_t *data = malloc(len + 1), *row = malloc(W), *sent = malloc(W);
    CHECK(data && row && sent);
    for (size_t i = 0; i < len; ++i) data[i] = (uint8_t)rnd();
    CHECK(demod_rs_frame_encode(data, len, h, crc, fec, row, (size_t)np - 1) == DEMOD_BUFFER_TOO_SMALL);
    CHECK(demod_rs_frame_encode(data, len, h, crc, fec, row, W) == np);
    for (size_t i = (size_t)np; i < W; ++i) row[i] = (uint8_t)rnd();
    memcpy(sent, row, W);
    const size_t c = crc == DEMOD_CRC16_CCITT_FALSE ? 2 : 4, n = (size_t)h + len + c;
    const unsigned D = (unsigned)(((size_t)np - n) / P);
    CHECK(demod_rs_max_len(W, h, crc, fec) >= (long long)len);
    for (unsigned j = 0; j < D; ++j) {
        /* distinct symbols of codeword j, the header bytes spared */
        const unsigned kj = (unsigned)((n - j + D - 1) / D), N = kj + P;
        uint8_t used[255] = {0};
        for (unsigned e = 0; e < wrong;) {
            const unsigned x = rnd() % N;
            const size_t at = x < kj ? j + (size_t)x * D : n + (size_t)(x - kj) * D + j;
            if (used[x] || at < (size_t)h) {
                if (N - (unsigned)h <= wrong) break;
                continue;
            }
            used[x] = 1;
            row[at] ^= (uint8_t)(1 + rnd() % 255);
            ++e;
        }
    }
    demod_frame_rs_t rec;
    const int rc = demod_rs_frame_decode(row, W, h, crc, fec, &rec);
    CHECK(rc == np && rec.codewords == D);
    CHECK(memcmp(row + np, sent + np, W - (size_t)np) == 0);
    if (wrong <= t) {
        CHECK(rec.status == DEMOD_RS_OK && rec.failed == 0 && memcmp(row, sent, (size_t)np) == 0);
        CHECK(demod_crc(crc, row, n - c) == (c == 2 ? (uint32_t)row[n - 2] << 8 | row[n - 1]
                                                    : (uint32_t)row[n - 4] << 24 | (uint32_t)row[n - 3] << 16 |
                                                          (uint32_t)row[n - 2] << 8 | row[n - 1]));
    } else {
        CHECK(rec.status == DEMOD_RS_OK || rec.status == DEMOD_RS_FAILED);
        CHECK((rec.status == DEMOD_RS_FAILED) == (rec.failed != 0) && rec.failed <= D);
    }
    free(data);
    free(row);
    free(sent);
}

static void random_rows(void)
{
    for (int it = 0; it < 200; ++it) {
        const int h = 1 + (int)(rnd() & 1), crc = 1 + (int)(rnd() & 1), fec = rnd() & 1 ? DEMOD_FEC_RS16 : DEMOD_FEC_RS32;
        const size_t W = 40 + rnd() % 900;
        uint8_t *row = malloc(W), *before = malloc(W);
        CHECK(row && before);
        for (size_t i = 0; i < W; ++i) row[i] = (uint8_t)rnd();
        if (h == 2) row[0] &= 3;
        memcpy(before, row, W);
        demod_frame_rs_t rec;
        const int rc = demod_rs_frame_decode(row, W, h, crc, fec, &rec);
        CHECK(rc >= h && (size_t)rc <= W);
        CHECK(memcmp(row + rc, before + rc, W - (size_t)rc) == 0);
        if (rec.status == DEMOD_RS_BAD_LENGTH) CHECK(rc == h && memcmp(row, before, W) == 0);
        free(row);
        free(before);
    }
}

static void refusals(void)
{
    static const int bad[] = {0, 2, 0x10, 0x31, 0x81, 0x300, 0x301, 0x400};
    uint8_t row[64] = {0}, out[64];
    demod_frame_rs_t rec;
    demod_frame_decode_t dec;
    int8_t soft[512] = {0};
    for (size_t i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
        const int f = bad[i];
        CHECK(demod_rs_frame_size(0, 1, 1, f) == DEMOD_BAD_ARG && demod_rs_max_len(64, 1, 1, f) == DEMOD_BAD_ARG);
        CHECK(demod_rs_frame_encode(NULL, 0, 1, 1, f, out, 64) == DEMOD_BAD_ARG);
        CHECK(demod_rs_frame_decode(row, 64, 1, 1, f, &rec) == DEMOD_BAD_ARG);
        CHECK(demod_fec_frame_symbols(0, 1, 1, 1, f) == DEMOD_BAD_ARG && demod_fec_air_index(f, 0) == DEMOD_BAD_ARG);
        CHECK(demod_fec_frame_encode(NULL, 0, 1, 1, f, out, 64) == DEMOD_BAD_ARG);
        CHECK(demod_fec_row_bytes(512, 1, 1, f) == DEMOD_BAD_ARG);
        CHECK(demod_fec_frame_decode(soft, 512, 1, 1, f, row, 64, &dec) == DEMOD_BAD_ARG);
    }
    /* the trellis's functions refuse a mode without the convolutional code */
    CHECK(demod_fec_frame_symbols(0, 1, 1, 1, DEMOD_FEC_RS16) == DEMOD_BAD_ARG);
    CHECK(demod_fec_air_index(DEMOD_FEC_RS32, 0) == DEMOD_BAD_ARG);
    /* rows too narrow for the shortest frame, and too wide for the payload limit */
    CHECK(demod_rs_max_len(18, 1, 1, DEMOD_FEC_RS16) == DEMOD_BAD_ARG && demod_rs_max_len(19, 1, 1, DEMOD_FEC_RS16) == 0);
    CHECK(demod_rs_frame_decode(row, 18, 1, 1, DEMOD_FEC_RS16, &rec) == DEMOD_BAD_ARG);
    CHECK(demod_rs_frame_decode(NULL, 64, 1, 1, DEMOD_FEC_RS16, &rec) == DEMOD_BAD_ARG);
    CHECK(demod_rs_frame_decode(row, 64, 3, 1, DEMOD_FEC_RS16, &rec) == DEMOD_BAD_ARG);
    CHECK(demod_rs_frame_decode(row, 64, 1, 3, DEMOD_FEC_RS16, &rec) == DEMOD_BAD_ARG);
    uint8_t *wide = calloc(1, 5000);
    CHECK(wide && demod_rs_frame_decode(wide, 5000, 2, 1, DEMOD_FEC_RS16, &rec) == DEMOD_BAD_ARG);
    free(wide);
}

/* one frame through encoder, hard soft values, Viterbi, outer decoder: the
 * burst that the convolutional code alone cannot take is repaired */
static void coded_chain(int fec, size_t burst)
{
    uint8_t data[100], air[1024], row[256];
    for (size_t i = 0; i < sizeof(data); ++i) data[i] = (uint8_t)rnd();
    const int nb = demod_fec_frame_encode(data, sizeof(data), 1, DEMOD_CRC16_CCITT_FALSE, fec, air, sizeof(air));
    CHECK(nb > 0);
    const long long S = demod_fec_frame_symbols(sizeof(data), 1, DEMOD_CRC16_CCITT_FALSE, 1, fec);
    CHECK(S > 0 && (S + 7) / 8 == nb);
    const size_t C = (size_t)S + 300;
    int8_t *soft = malloc(C);
    CHECK(soft);
    for (size_t i = 0; i < C; ++i)
        soft[i] = i < (size_t)S ? (((air[i >> 3] >> (7 - (i & 7))) & 1) ? -127 : 127) : (int8_t)(rnd() % 255 - 127);
    for (size_t i = 400; i < 400 + burst; ++i) soft[i] = (int8_t)-soft[i];
    const long long Bd = demod_fec_row_bytes(C, 1, 1, fec);
    CHECK(Bd > 0 && Bd <= (long long)sizeof(row));
    demod_frame_decode_t dec;
    const long long np = demod_rs_frame_size(sizeof(data), 1, DEMOD_CRC16_CCITT_FALSE, fec);
    CHECK(demod_fec_frame_decode(soft, C, 1, DEMOD_CRC16_CCITT_FALSE, fec, row, (size_t)Bd, &dec) == np);
    CHECK(dec.status == DEMOD_DECODE_OK && dec.length == sizeof(data) && dec.steps == 8 * (unsigned)np + 6);
    demod_frame_rs_t rec;
    CHECK(demod_rs_frame_decode(row, (size_t)Bd, 1, DEMOD_CRC16_CCITT_FALSE, fec, &rec) == np);
    CHECK(rec.status == DEMOD_RS_OK && memcmp(row + 1, data, sizeof(data)) == 0);
    free(soft);
}

int main(int argc, char **argv)
{
    rng_state = argc > 1 ? strtoull(argv[1], NULL, 0) : 1;
    pins();
    for (int fec = DEMOD_FEC_RS16; fec <= DEMOD_FEC_RS32; fec <<= 1) {
        const unsigned P = fec == DEMOD_FEC_RS16 ? 16 : 32, t = P / 2, kmax = 255 - P;
        for (int h = 1; h <= 2; ++h)
            for (int crc = 1; crc <= 2; ++crc) {
                const size_t c = crc == 1 ? 2 : 4;
                size_t lens[6] = {0, 1, kmax - (size_t)h - c, kmax - (size_t)h - c + 1, 0, 0};
                size_t nl = 4;
                if (h == 2) {
                    lens[nl++] = 2 * kmax + 2 - (size_t)h - c;
                    lens[nl++] = DEMOD_MAX_FRAME_PAYLOAD;
                }
                for (size_t li = 0; li < nl; ++li)
                    for (unsigned wrong = 0; wrong <= t + 1; wrong += wrong < 1 ? 1 : (wrong < t ? t - 1 : 1))
                        one_frame(lens[li], h, crc, fec, wrong, li & 1 ? 0 : 5);
            }
        coded_chain(DEMOD_FEC_CONV_K7 | fec, 40);
        coded_chain(DEMOD_FEC_CONV_K7 | DEMOD_FEC_RATE_3_4 | DEMOD_FEC_INTERLEAVE | fec, 8);
    }
    random_rows();
    refusals();
    puts("rs_host_test OK");
    return 0;
}
