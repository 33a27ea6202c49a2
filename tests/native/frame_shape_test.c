/*
 * frame_shape_test.c — csrc/frame_shape.h and the launch arithmetic of
 * csrc/frame_rows.h in a program of its own, built with
 * -fsanitize=address,undefined by tests/test_frame_shape_cpu.py together with
 * the library's host C files (no device code, no shared library). The
 * headers' closed forms are held to counts written here from the definitions
 * (include/demod.h):
 *
 *   St       the greatest T with Nt(T) <= Cu, Nt counted step by step from the
 *            puncturing pattern, Cu whole interleaver blocks with the flag
 *   max_len  the greatest len with n'(h + len + c) <= W, n' counted codeword
 *            by codeword
 *   span     the symbols of a frame on the air: its n' bytes' bits, or T =
 *            max(8 n' + 6, 8 h + DEMOD_FEC_DEPTH) steps, Nt(T) kept bits, whole
 *            interleaver blocks with the flag
 *   wpg      min(want, max(16384 / n_groups, 1)) waves a group, and the
 *            workgroups of four waves that hold them
 *
 * St and max_len are monotone in N, so a sweep of N upward advances them step
 * by step. Every N from 0 to eight past the first one refused for a max_len
 * beyond DEMOD_MAX_FRAME_PAYLOAD, for fec 0 and the 20 modes, bits 1 .. 4, h 1
 * and 2 and both CRC kinds; then the refusals of what is no shape at all. The
 * span at every len from 0 to DEMOD_MAX_FRAME_PAYLOAD in the same modes, also
 * against the public functions that are expressed through it.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../audio-network_amd/csrc/frame_rows.h"
#include "../../audio-network_amd/csrc/frame_shape.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: %s (fec 0x%x bits %d h %d crc %d N %lu)\n", __FILE__, __LINE__, #c, \
                    (unsigned)g_fec, g_bits, g_h, g_crc, (unsigned long)g_N);  \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

static int g_fec, g_bits, g_h, g_crc;
static size_t g_N;

/* the coded bits step t keeps: the pattern of include/demod.h, by step phase */
static unsigned kept_in_step(int conv, unsigned long t)
{
    if (conv & DEMOD_FEC_RATE_2_3) return t % 2 == 0 ? 2 : 1;
    if (conv & DEMOD_FEC_RATE_3_4) return t % 3 == 0 ? 2 : 1;
    return 2;
}

/* n' of a frame of n bytes: its message bytes dealt to codewords of at most
 * 255 - P, P parity bytes each */
static unsigned long protected_bytes(unsigned long n, unsigned P)
{
    if (!P) return n;
    unsigned long total = n;
    for (unsigned long left = n; left > 0; left -= left < 255 - P ? left : 255 - P) total += P;
    return total;
}

static unsigned long codewords(unsigned long n, unsigned P) { return P ? (protected_bytes(n, P) - n) / P : 0; }

/* one (mode, bits, h, crc): returns the N swept */
static unsigned long sweep(int fec, int bits, int h, int crc)
{
    const int conv = fec & 0xFF, P = fec & DEMOD_FEC_RS16 ? 16 : fec & DEMOD_FEC_RS32 ? 32 : 0;
    const unsigned long c = crc == DEMOD_CRC16_CCITT_FALSE ? 2 : 4, least = 8 * (unsigned long)h + DEMOD_FEC_DEPTH;
    unsigned long T = 0, NtT = 0;   /* St and Nt(St) so far */
    long len = -1;                  /* max_len so far: -1, no frame fits */
    unsigned long past = 0, first_ok = 0, n_ok = 0;
    g_fec = fec, g_bits = bits, g_h = h, g_crc = crc;
    for (size_t N = 0;; ++N) {
        g_N = N;
        const unsigned long C = (unsigned long)N * (unsigned long)bits;
        unsigned long W = (C + 7) / 8;
        int refused = 0;
        if (conv) {
            const unsigned long Cu = conv & DEMOD_FEC_INTERLEAVE ? C / 256 * 256 : C;
            while (NtT + kept_in_step(conv, T) <= Cu) NtT += kept_in_step(conv, T++);
            CHECK(frame_row_steps((unsigned)conv, C) == T);
            refused = T < least;
            W = refused ? 0 : (T - 6) / 8;
        }
        while (!refused && protected_bytes((unsigned long)h + (unsigned long)(len + 1) + c, (unsigned)P) <= W) ++len;
        const int too_long = !refused && len > DEMOD_MAX_FRAME_PAYLOAD;
        refused |= len < 0 || too_long;

        struct frame_shape s;
        const int rc = frame_shape_fill(&s, bits, 1, N, h, crc, fec);
        CHECK((rc != 0) == refused);
        if (!refused) {
            CHECK(s.row_bytes == W && s.max_len == (unsigned long)len && s.steps == (conv ? T : 0));
            CHECK(s.len_bytes == h && s.crc_bytes == (int)c && s.bits == bits);
            CHECK(s.fec == conv && s.fec_depth == (conv ? DEMOD_FEC_DEPTH : 0) && s.parity == P);
            CHECK(frame_max_len((unsigned)W, (unsigned)h, (unsigned)c, (unsigned)P) == len);
            /* the frame of max_len fills whole codewords' worth of the row, the next one does not fit */
            CHECK(codewords((unsigned long)h + (unsigned long)len + c, (unsigned)P) ==
                  rs_codewords((unsigned)(h + len) + (unsigned)c, (unsigned)P));
            if (!n_ok++) first_ok = N;
        }
        /* a coded mode needs K = 2^bits whatever else holds */
        if (conv) CHECK(frame_shape_fill(&s, bits, 0, N, h, crc, fec) != 0);
        if (too_long && ++past > 8) {
            CHECK(n_ok > 0 && first_ok < N);
            return N + 1;
        }
    }
}

/* the span of every len in one (mode, bits, h, crc): returns the calls compared */
static unsigned long span_sweep(int fec, int bits, int h, int crc)
{
    const int conv = fec & 0xFF, P = fec & DEMOD_FEC_RS16 ? 16 : fec & DEMOD_FEC_RS32 ? 32 : 0;
    const unsigned long c = crc == DEMOD_CRC16_CCITT_FALSE ? 2 : 4;
    unsigned long calls = 0, Tc = 0, NtTc = 0;   /* Nt counted step by step: T does not fall as len grows */
    demod_tx_cfg_t x = {.sync_len = 5, .len_bytes = (uint32_t)h, .crc = (uint32_t)crc, .fec = (uint32_t)fec,
                        .max_len = DEMOD_MAX_FRAME_PAYLOAD};
    g_fec = fec, g_bits = bits, g_h = h, g_crc = crc;
    for (size_t len = 0; len <= DEMOD_MAX_FRAME_PAYLOAD; ++len) {
        g_N = len;
        const unsigned long np = protected_bytes((unsigned long)h + len + c, (unsigned)P);
        unsigned long T = 0, Nt = 0, air = 8 * np;
        if (conv) {
            T = 8 * np + 6 > 8 * (unsigned long)h + DEMOD_FEC_DEPTH ? 8 * np + 6 : 8 * (unsigned long)h + DEMOD_FEC_DEPTH;
            while (Tc < T) NtTc += kept_in_step(conv, Tc++);
            CHECK(Tc == T);
            Nt = NtTc;
            air = conv & DEMOD_FEC_INTERLEAVE ? (Nt + DEMOD_FEC_IL_ROWS * DEMOD_FEC_IL_COLS - 1) / 256 * 256 : Nt;
            if (!(conv & (DEMOD_FEC_RATE_2_3 | DEMOD_FEC_RATE_3_4 | DEMOD_FEC_INTERLEAVE)))   /* the unmapped mode */
                CHECK(2 * T == fec_air_bits((unsigned)conv, fec_kept_bits((unsigned)conv, (unsigned)T)));
        }
        const unsigned long want = (air + (unsigned long)bits - 1) / (unsigned long)bits;
        unsigned steps = 77, kept = 77;
        CHECK(frame_air_symbols((unsigned)len, (unsigned)h, (unsigned)c, (unsigned)bits, (unsigned)conv, (unsigned)P,
                                &steps, &kept) == want);
        CHECK(steps == T && kept == Nt);
        ++calls;
        /* the public functions: they refuse a len that h bytes cannot say, the arithmetic does not */
        const int fits = len <= (h == 1 ? 0xFFu : 0xFFFFu);
        const long long n = demod_checked_frame_size(len, h, crc);
        CHECK(n == (fits ? (long long)((unsigned long)h + len + c) : DEMOD_FRAME_TOO_LARGE));
        if (fec == DEMOD_FEC_CONV_K7 && bits == 1)
            CHECK(demod_coded_frame_steps(len, h, crc) == (fits ? (long long)T : DEMOD_FRAME_TOO_LARGE));
        if (conv)
            CHECK(demod_fec_frame_symbols(len, h, crc, bits, fec) == (fits ? (long long)want : DEMOD_FRAME_TOO_LARGE));
        /* K = 2^bits tones; fec 0, the plain mode, runs the uncoded branch as the parity-only modes do */
        CHECK(demod_tx_frame_symbol_count(&x, 1u << bits, len) == (fits ? (long long)(5 + want) : DEMOD_FRAME_TOO_LARGE));
        calls += 3 + (conv != 0);
    }
    return calls;
}

/* row_waves_per_group and row_blocks against include/demod.h's formula */
static void launches(void)
{
    static const unsigned groups[] = {1, 2, 4096, 5461, 8193, 16383, 16384, 16385, 65536};
    static const unsigned long long wants[] = {1, 2, 3, 4, 5, 16384, 16385, 0x7FFFFFFF};
    g_fec = g_bits = g_h = g_crc = 0;
    for (size_t i = 0; i < sizeof(groups) / sizeof(groups[0]); ++i)
        for (size_t j = 0; j < sizeof(wants) / sizeof(wants[0]); ++j) {
            const unsigned long long S = groups[i], most = 16384 / S > 1 ? 16384 / S : 1;
            const unsigned long long wpg = wants[j] < most ? wants[j] : most;
            g_N = (size_t)S;
            CHECK(row_waves_per_group(groups[i], wants[j]) == wpg);
            CHECK(row_blocks(groups[i], (unsigned)wpg) == (S * wpg + 3) / 4);
            CHECK(S * wpg <= (S > 16384 ? S : 16384) && wpg >= 1);
        }
    CHECK(kRowThreads == 256 && kRowLanes == 64 && kRowWaves == 4 && kRowMaxWaves == 16384);
}

static void refusals(void)
{
    static const int bad[] = {2,     0x10,  0x20,  0x30,  0x31,  0x81,  0x41 | 0x30, 0x300,
                              0x301, 0x311, 0x110, 0x220, 0x400, 0x401, -1};
    struct frame_shape s;
    g_bits = 2, g_h = 1, g_crc = 1, g_N = 400;
    for (size_t i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
        g_fec = bad[i];
        CHECK(!rs_mode_valid((unsigned)bad[i]));
        CHECK(frame_shape_fill(&s, 2, 1, 400, 1, DEMOD_CRC16_CCITT_FALSE, bad[i]) != 0);
    }
    /* K = 3: two bits a symbol, no power of two. Refused with the convolutional code alone */
    static const int modes[] = {0, DEMOD_FEC_RS16, DEMOD_FEC_RS32, DEMOD_FEC_CONV_K7, DEMOD_FEC_CONV_K7 | DEMOD_FEC_RS16,
                                DEMOD_FEC_CONV_K7 | DEMOD_FEC_RATE_3_4 | DEMOD_FEC_INTERLEAVE | DEMOD_FEC_RS32};
    for (size_t i = 0; i < sizeof(modes) / sizeof(modes[0]); ++i) {
        g_fec = modes[i];
        CHECK(frame_shape_fill(&s, 2, 1, 400, 1, DEMOD_CRC16_CCITT_FALSE, modes[i]) == 0);
        CHECK((frame_shape_fill(&s, 2, 0, 400, 1, DEMOD_CRC16_CCITT_FALSE, modes[i]) != 0) == ((modes[i] & 0xFF) != 0));
    }
    g_fec = 0;
    CHECK(frame_shape_fill(&s, 2, 1, 400, 0, DEMOD_CRC16_CCITT_FALSE, 0) != 0);
    CHECK(frame_shape_fill(&s, 2, 1, 400, 3, DEMOD_CRC16_CCITT_FALSE, 0) != 0);
    CHECK(frame_shape_fill(&s, 2, 1, 400, 1, 0, 0) != 0 && frame_shape_fill(&s, 2, 1, 400, 1, 3, 0) != 0);
    CHECK(frame_shape_fill(&s, 2, 1, (size_t)0x7FFFFFFF + 1, 1, DEMOD_CRC16_CCITT_FALSE, 0) != 0);
    CHECK(frame_shape_fill(&s, 4, 1, (size_t)0x7FFFFFFF, 2, DEMOD_CRC32_MPEG2, DEMOD_FEC_CONV_K7 | DEMOD_FEC_RATE_2_3) != 0);
    CHECK(frame_crc_bytes(DEMOD_CRC16_CCITT_FALSE) == 2 && frame_crc_bytes(DEMOD_CRC32_MPEG2) == 4);
    CHECK(frame_crc_bytes(0) == 0 && frame_crc_bytes(3) == 0 && frame_crc_bytes(-1) == 0);
    /* air bits beyond 32 bits: the identity map halves them, a mapped mode has no such row */
    CHECK(frame_row_steps(DEMOD_FEC_CONV_K7, 0x1FFFFFFFCull) == 0xFFFFFFFEull);
    CHECK(frame_row_steps(DEMOD_FEC_CONV_K7 | DEMOD_FEC_RATE_2_3, 0xFFFFFFFFull) == 2ull * (0xFFFFFFFFull / 3));
    CHECK(frame_row_steps(DEMOD_FEC_CONV_K7 | DEMOD_FEC_RATE_2_3, 0x100000000ull) == 0);
    CHECK(frame_row_steps(DEMOD_FEC_CONV_K7 | DEMOD_FEC_INTERLEAVE, 0x100000000ull) == 0);
}

int main(void)
{
    static const int convs[] = {0,
                                DEMOD_FEC_CONV_K7,
                                DEMOD_FEC_CONV_K7 | DEMOD_FEC_RATE_2_3,
                                DEMOD_FEC_CONV_K7 | DEMOD_FEC_RATE_3_4,
                                DEMOD_FEC_CONV_K7 | DEMOD_FEC_INTERLEAVE,
                                DEMOD_FEC_CONV_K7 | DEMOD_FEC_RATE_2_3 | DEMOD_FEC_INTERLEAVE,
                                DEMOD_FEC_CONV_K7 | DEMOD_FEC_RATE_3_4 | DEMOD_FEC_INTERLEAVE};
    static const int flags[] = {0, DEMOD_FEC_RS16, DEMOD_FEC_RS32};
    unsigned long shapes = 0, combos = 0, spans = 0;
    for (size_t m = 0; m < sizeof(convs) / sizeof(convs[0]); ++m)
        for (size_t f = 0; f < sizeof(flags) / sizeof(flags[0]); ++f) {
            const int fec = convs[m] | flags[f];
            g_fec = fec, g_N = 0;
            CHECK(fec == 0 || rs_mode_valid((unsigned)fec));
            for (int bits = 1; bits <= 4; ++bits)
                for (int h = 1; h <= 2; ++h)
                    for (int crc = DEMOD_CRC16_CCITT_FALSE; crc <= DEMOD_CRC32_MPEG2; ++crc, ++combos) {
                        shapes += sweep(fec, bits, h, crc);
                        spans += span_sweep(fec, bits, h, crc);
                    }
        }
    refusals();
    launches();
    printf("frame_shape_test OK: %lu combinations, %lu shapes, %lu span calls\n", combos, shapes, spans);
    return 0;
}
