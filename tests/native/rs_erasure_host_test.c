/*
 * rs_erasure_host_test.c — the host side of erasure decoding (demod_rs.c's
 * demod_rs_frame_decode_erasures, demod_fec.c's demod_soft_erasures) in a
 * program of its own, built with -fsanitize=address,undefined by
 * tests/test_rs_erasures_cpu.py: every frame shape with f flagged and e other
 * wrong bytes a codeword, 2 e + f <= P (which must come back), masks and errors
 * of any weight in rows of exactly W bytes and masks of exactly Wm words (which
 * must not touch a byte past the frame or read a word past the mask), the NULL
 * mask against demod_rs_frame_decode, the mask from soft values, the refusals.
 *
 *   rs_erasure_host_test [seed]
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

static unsigned parity_of(int fec) { return fec & DEMOD_FEC_RS16 ? 16u : 32u; }

/* heap copies of exactly the sizes the decoder may touch */
static uint8_t *row_of(const uint8_t *src, size_t W)
{
    uint8_t *p = (uint8_t *)malloc(W);
    CHECK(p);
    memcpy(p, src, W);
    return p;
}

static uint64_t *mask_of(size_t W)
{
    uint64_t *m = (uint64_t *)calloc((W + 63) / 64, sizeof(uint64_t));
    CHECK(m);
    return m;
}

static void flag(uint64_t *m, size_t b) { m[b >> 6] |= (uint64_t)1 << (b & 63); }

/* f flagged (every second one wrong) and e other wrong bytes in every codeword of a frame of len bytes */
static void one_frame(size_t len, int h, int crc, int fec, unsigned f, unsigned e, size_t pad)
{
    const unsigned P = parity_of(fec);
    uint8_t data[DEMOD_MAX_FRAME_PAYLOAD], sent[4800];
    for (size_t i = 0; i < len; ++i) data[i] = (uint8_t)rnd();
    const int np = demod_rs_frame_encode(data, len, h, crc, fec, sent, sizeof(sent));
    CHECK(np > 0);
    const size_t W = (size_t)np + pad;
    memset(sent + np, 0xEE, pad);
    uint8_t *row = row_of(sent, W);
    uint64_t *mask = mask_of(W);
    const unsigned c = crc == DEMOD_CRC16_CCITT_FALSE ? 2u : 4u, n = (unsigned)h + (unsigned)len + c;
    const unsigned D = (n + (254u - P)) / (255u - P);
    unsigned planted = 0;
    for (unsigned j = 0; j < D; ++j) {
        const unsigned kj = (n - j + D - 1u) / D, N = kj + P;
        uint8_t used[255] = {0};
        unsigned ff = f < N ? f : N, ee = e;
        if (ff + ee > N - 2u) ee = N - 2u > ff ? N - 2u - ff : 0;   /* room, the header's symbols spared */
        for (unsigned i = 0; i < ff + ee; ++i) {
            unsigned x;
            do x = rnd() % N;
            while (used[x] || (x < kj && j + x * D < (unsigned)h && i >= ff));
            used[x] = 1;
            const unsigned off = x < kj ? j + x * D : n + (x - kj) * D + j;
            const int header = off < (unsigned)h;
            if (i < ff) {
                flag(mask, off);
                ++planted;
            }
            if (!header && (i >= ff || (i & 1u))) row[off] ^= (uint8_t)(1u + rnd() % 255u);
        }
    }
    for (size_t b = (size_t)np; b < W; ++b) flag(mask, b);   /* past n': ignored */
    demod_frame_rs_t rec;
    demod_frame_erase_t erec;
    const int covered = demod_rs_frame_decode_erasures(row, W, h, crc, fec, mask, &rec, &erec);
    CHECK(covered == np);
    CHECK(rec.codewords == D && erec.reserved == 0 && erec.erased == planted);
    if (2u * e + f <= P) {
        CHECK(rec.status == DEMOD_RS_OK && rec.failed == 0);
        CHECK(memcmp(row, sent, W) == 0);
        CHECK(erec.fallback == 0 || f == 0);
    } else {
        CHECK(memcmp(row + np, sent + np, pad) == 0);
    }
    free(mask);
    free(row);
}

static void random_rows(int fec, unsigned rounds)
{
    for (unsigned r = 0; r < rounds; ++r) {
        const int h = 1 + (int)(rnd() & 1u), crc = (rnd() & 1u) ? DEMOD_CRC16_CCITT_FALSE : DEMOD_CRC32_MPEG2;
        const size_t W = 40 + rnd() % 700;
        uint8_t *row = (uint8_t *)malloc(W), *copy;
        uint64_t *mask = mask_of(W);
        CHECK(row);
        for (size_t b = 0; b < W; ++b) {
            row[b] = (uint8_t)rnd();
            if (rnd() % 8u == 0) flag(mask, b);
        }
        if (h == 2) row[0] = (uint8_t)(rnd() % 3u);
        copy = row_of(row, W);
        demod_frame_rs_t rec, rec0;
        demod_frame_erase_t erec;
        const int covered = demod_rs_frame_decode_erasures(row, W, h, crc, fec, mask, &rec, &erec);
        CHECK(covered > 0 && (size_t)covered <= W);
        CHECK(memcmp(row + covered, copy + covered, W - (size_t)covered) == 0);
        CHECK(erec.used + erec.fallback <= rec.codewords && erec.reserved == 0);
        if (rec.status == DEMOD_RS_BAD_LENGTH) CHECK(covered == h && erec.erased == 0 && memcmp(row, copy, W) == 0);
        /* a NULL mask is the plain decoder */
        memcpy(row, copy, W);
        const int c1 = demod_rs_frame_decode_erasures(row, W, h, crc, fec, NULL, &rec, &erec);
        const int c0 = demod_rs_frame_decode(copy, W, h, crc, fec, &rec0);
        CHECK(c1 == c0 && memcmp(row, copy, W) == 0 && memcmp(&rec, &rec0, sizeof(rec)) == 0);
        CHECK(erec.erased == 0 && erec.used == 0 && erec.fallback == 0);
        free(copy);
        free(mask);
        free(row);
    }
}

static void soft_masks(void)
{
    for (unsigned r = 0; r < 50; ++r) {
        const size_t n_soft = 1 + rnd() % 900, row_bytes = 1 + rnd() % 130;
        const int level = 1 + (int)(rnd() % 127u);
        int8_t *soft = (int8_t *)malloc(n_soft);
        uint64_t *mask = (uint64_t *)malloc((row_bytes + 63) / 64 * sizeof(uint64_t));
        CHECK(soft && mask);
        for (size_t m = 0; m < n_soft; ++m) soft[m] = (int8_t)(rnd() % 255u) - 127;
        CHECK(demod_soft_erasures(soft, n_soft, level, mask, row_bytes) == (int)((row_bytes + 63) / 64));
        for (size_t b = 0; b < (row_bytes + 63) / 64 * 64; ++b) {
            int least = 128;
            for (size_t m = 8 * b; m < 8 * b + 8; ++m) {
                const int q = m < n_soft ? soft[m] : 0, a = q < 0 ? -q : q;
                if (a < least) least = a;
            }
            CHECK((int)((mask[b >> 6] >> (b & 63)) & 1u) == (b < row_bytes && least < level));
        }
        free(mask);
        free(soft);
    }
}

static void refusals(void)
{
    uint8_t row[64] = {0};
    uint64_t mask[2] = {0, 0};
    int8_t soft[64] = {0};
    demod_frame_rs_t rec;
    demod_frame_erase_t erec;
    const int fec = DEMOD_FEC_RS16, crc = DEMOD_CRC16_CCITT_FALSE;
    CHECK(demod_rs_frame_decode_erasures(row, 64, 1, crc, fec, mask, &rec, &erec) == 19);
    CHECK(demod_rs_frame_decode_erasures(NULL, 64, 1, crc, fec, mask, &rec, &erec) == DEMOD_BAD_ARG);
    CHECK(demod_rs_frame_decode_erasures(row, 64, 1, crc, fec, mask, NULL, &erec) == DEMOD_BAD_ARG);
    CHECK(demod_rs_frame_decode_erasures(row, 64, 1, crc, fec, mask, &rec, NULL) == DEMOD_BAD_ARG);
    CHECK(demod_rs_frame_decode_erasures(row, 64, 1, crc, fec, (const uint64_t *)((const char *)mask + 4), &rec,
                                         &erec) == DEMOD_BAD_ARG);
    CHECK(demod_rs_frame_decode_erasures(row, 64, 1, crc, DEMOD_FEC_CONV_K7, mask, &rec, &erec) == DEMOD_BAD_ARG);
    CHECK(demod_rs_frame_decode_erasures(row, 64, 1, crc, fec | DEMOD_FEC_ERASE(16), mask, &rec, &erec) ==
          DEMOD_BAD_ARG);
    CHECK(demod_rs_frame_decode_erasures(row, 64, 3, crc, fec, mask, &rec, &erec) == DEMOD_BAD_ARG);
    CHECK(demod_rs_frame_decode_erasures(row, 10, 1, crc, fec, mask, &rec, &erec) == DEMOD_BAD_ARG);
    CHECK(demod_rs_frame_size(0, 1, crc, fec | DEMOD_FEC_ERASE(16)) == DEMOD_BAD_ARG);
    CHECK(demod_soft_erasures(soft, 64, 1, mask, 8) == 1 && mask[0] == 0xFF);
    CHECK(demod_soft_erasures(soft, 64, 0, mask, 8) == DEMOD_BAD_ARG);
    CHECK(demod_soft_erasures(soft, 64, 128, mask, 8) == DEMOD_BAD_ARG);
    CHECK(demod_soft_erasures(NULL, 64, 1, mask, 8) == DEMOD_BAD_ARG);
    CHECK(demod_soft_erasures(soft, 64, 1, NULL, 8) == DEMOD_BAD_ARG);
    CHECK(demod_soft_erasures(soft, 64, 1, (uint64_t *)((char *)mask + 4), 8) == DEMOD_BAD_ARG);
    CHECK(demod_soft_erasures(soft, 64, 1, mask, 0) == DEMOD_BAD_ARG);
}

int main(int argc, char **argv)
{
    rng_state = argc > 1 ? (uint64_t)strtoull(argv[1], NULL, 10) : 1;
    static const int fecs[4] = {DEMOD_FEC_RS16, DEMOD_FEC_RS32, DEMOD_FEC_RS16 | DEMOD_FEC_CONV_K7,
                                DEMOD_FEC_RS32 | DEMOD_FEC_CONV_K7 | DEMOD_FEC_RATE_3_4 | DEMOD_FEC_INTERLEAVE};
    static const size_t lens[6] = {0, 1, 200, 250, 700, DEMOD_MAX_FRAME_PAYLOAD};
    for (int m = 0; m < 4; ++m) {
        const unsigned P = parity_of(fecs[m]);
        for (int l = 0; l < 6; ++l) {
            const int h = lens[l] > 255 ? 2 : 1 + (l & 1);
            const int crc = (l & 1) ? DEMOD_CRC32_MPEG2 : DEMOD_CRC16_CCITT_FALSE;
            const size_t pad = lens[l] == DEMOD_MAX_FRAME_PAYLOAD ? 0 : 3;
            const unsigned fs[7] = {0, 1, 2, P / 2, P - 1, P, P + 1};
            for (int i = 0; i < 7; ++i) {
                const unsigned f = fs[i];
                const unsigned most = f <= P ? (P - f) / 2 : 0;
                one_frame(lens[l], h, crc, fecs[m], f, most, pad);
                one_frame(lens[l], h, crc, fecs[m], f, most + 1, pad);
                if (most) one_frame(lens[l], h, crc, fecs[m], f, 0, pad);
            }
        }
        random_rows(fecs[m], 60);
    }
    soft_masks();
    refusals();
    printf("rs_erasure_host_test OK\n");
    return 0;
}
