/*
 * demod_rs.c — the host side of the Reed-Solomon outer code (include/demod.h
 * "Reed-Solomon outer code", DESIGN.md §4.9 "Reed-Solomon outer code"): the
 * systematic encoder over a checked frame's bytes and the bounded-distance
 * decoder the device stage (frames_rs.hip) is held to, bit for bit. Field,
 * layout and modes are rs_ops.h's. Integer arithmetic alone, no allocation.
 * Pure host work, no device.
 *
 * The decoder of one codeword: syndromes by Horner, Berlekamp-Massey for the
 * locator, a search of the codeword's own positions for its roots, Forney for
 * the values. It accepts only a locator of degree L <= t with L roots among
 * the k_j + P positions and non-zero values; the sequence a locator with L
 * distinct roots generates is a sum of L exponentials, so the word it leaves
 * has zero syndromes and lies within t of the received one: the unique such
 * codeword. Everything else leaves the bytes alone and counts as failed.
 *
 * With an erasure mask (include/demod.h "erasure decoding",
 * demod_rs_frame_decode_erasures: the reference of the device stage's second
 * instantiation) a dirty codeword with 1 <= f <= P flagged positions first
 * goes through correct_errata, which finds the codeword with 2 e + f <= P or
 * nothing; on nothing, and with f > P, the errors-only decoder runs on the
 * same syndromes.
 */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "frame_shape.h"

static void build_tables(uint8_t *exp, uint8_t *log)
{
    unsigned v = 1;
    log[0] = 0;
    for (unsigned e = 0; e < 255; ++e, v = rs_xtime(v)) rs_table_entry(e, v, exp, log);
}

int demod_rs_generator(int parity_bytes, uint8_t *g)
{
    if (!g || parity_bytes < 1 || parity_bytes > RS_MAX_PARITY) return DEMOD_BAD_ARG;
    rs_generator((unsigned)parity_bytes, g);
    return parity_bytes + 1;
}

int demod_rs_encode(const uint8_t *msg, size_t k, int parity_bytes, uint8_t *parity)
{
    if (!msg || !parity || parity_bytes < 1 || parity_bytes > RS_MAX_PARITY || k == 0 ||
        k > 255u - (unsigned)parity_bytes)
        return DEMOD_BAD_ARG;
    uint8_t g[RS_MAX_PARITY + 1];
    rs_generator((unsigned)parity_bytes, g);
    rs_remainder(msg, (unsigned)k, 1, (unsigned)parity_bytes, g, parity);
    return parity_bytes;
}

long long demod_rs_frame_size(size_t len, int len_bytes, int crc, int fec)
{
    if (!rs_mode_valid((unsigned)fec)) return DEMOD_BAD_ARG;
    const long long n = demod_checked_frame_size(len, len_bytes, crc);
    if (n < 0) return n;
    return (long long)rs_frame_bytes((unsigned)n, rs_parity((unsigned)fec));
}

long long demod_rs_max_len(size_t row_bytes, int len_bytes, int crc, int fec)
{
    const int c = frame_crc_bytes(crc);
    if (!rs_mode_valid((unsigned)fec) || c == 0 || (len_bytes != 1 && len_bytes != 2) || row_bytes > 0x7FFFFFFF)
        return DEMOD_BAD_ARG;
    const long long m = frame_max_len((unsigned)row_bytes, (unsigned)len_bytes, (unsigned)c, rs_parity((unsigned)fec));
    return m < 0 ? DEMOD_BAD_ARG : m;
}

int demod_rs_frame_encode(const uint8_t *data, size_t len, int len_bytes, int crc, int fec, uint8_t *out,
                          size_t cap)
{
    const long long np = demod_rs_frame_size(len, len_bytes, crc, fec);
    if (np < 0) return (int)np;
    if ((!data && len) || !out) return DEMOD_BAD_ARG;
    if ((size_t)np > cap) return DEMOD_BUFFER_TOO_SMALL;
    const int n = demod_checked_frame_encode(data, len, len_bytes, crc, out, cap);
    if (n < 0) return n;
    rs_frame_protect(out, (unsigned)n, rs_parity((unsigned)fec));
    return (int)np;
}

/* S_i = r(alpha^i), i < P, by Horner; nonzero when one of them is */
static unsigned syndromes(const uint8_t *r, unsigned N, unsigned P, const uint8_t *exp, const uint8_t *log,
                          uint8_t *S)
{
    unsigned any = 0;
    for (unsigned i = 0; i < P; ++i) {
        unsigned s = 0;
        for (unsigned x = 0; x < N; ++x) s = rs_tscale(exp, log, s, i) ^ r[x];
        S[i] = (uint8_t)s;
        any |= s;
    }
    return any;
}

#define LOCATOR_SIZE (RS_MAX_PARITY + 2)

/* Berlekamp-Massey on S[0 .. count), count <= RS_MAX_PARITY: C the locator (all LOCATOR_SIZE coefficients
 * written, zero past its degree), B the one before the last length change. Returns L. */
static unsigned locator(const uint8_t *S, unsigned count, const uint8_t *exp, const uint8_t *log,
                        uint8_t C[LOCATOR_SIZE])
{
    uint8_t B[LOCATOR_SIZE], T[LOCATOR_SIZE];
    memset(C, 0, LOCATOR_SIZE);
    memset(B, 0, LOCATOR_SIZE);
    C[0] = B[0] = 1;
    unsigned L = 0, m = 1, b = 1;
    for (unsigned k = 0; k < count; ++k) {
        unsigned d = 0;
        for (unsigned l = 0; l <= L && l <= k; ++l) d ^= rs_tmul(exp, log, C[l], S[k - l]);
        if (d == 0) {
            ++m;
            continue;
        }
        const unsigned coef = rs_tdiv(exp, log, d, b);
        memcpy(T, C, LOCATOR_SIZE);
        for (unsigned l = m; l <= count; ++l) C[l] ^= (uint8_t)rs_tmul(exp, log, coef, B[l - m]);
        if (2 * L <= k) {
            L = k + 1 - L;
            memcpy(B, T, LOCATOR_SIZE);
            b = d;
            m = 1;
        } else {
            ++m;
        }
    }
    return L;
}

/* The errors-only rule on a word with the syndromes S, not all zero. */
static int correct_errors(uint8_t *r, unsigned N, unsigned P, const uint8_t *S, const uint8_t *exp,
                          const uint8_t *log)
{
    const unsigned t = P / 2;
    uint8_t C[LOCATOR_SIZE];
    const unsigned L = locator(S, P, exp, log, C);
    if (L > t) return -1;
    /* the roots among the codeword's own positions: x has X = alpha^(N - 1 - x) */
    unsigned pos[RS_MAX_T], found = 0;
    for (unsigned x = 0; x < N; ++x) {
        const unsigned z = (255u - (N - 1u - x)) % 255u;   /* X^-1 = alpha^z */
        unsigned v = C[L];
        for (unsigned l = L; l-- > 0;) v = rs_tscale(exp, log, v, z) ^ C[l];
        if (v == 0) {
            if (found == L) return -1;
            pos[found++] = x;
        }
    }
    if (found != L) return -1;
    /* Forney: omega = S(x) C(x) mod x^L, e = X omega(X^-1) / C'(X^-1) */
    uint8_t om[RS_MAX_T], val[RS_MAX_T];
    for (unsigned i = 0; i < L; ++i) {
        unsigned v = 0;
        for (unsigned l = 0; l <= i; ++l) v ^= rs_tmul(exp, log, C[l], S[i - l]);
        om[i] = (uint8_t)v;
    }
    for (unsigned e = 0; e < L; ++e) {
        const unsigned p = N - 1u - pos[e], z = (255u - p) % 255u, z2 = (2u * z) % 255u;
        unsigned num = 0, den = 0;
        for (unsigned i = L; i-- > 0;) num = rs_tscale(exp, log, num, z) ^ om[i];
        for (unsigned l = (L & 1u) ? L : L - 1u;; l -= 2) {   /* the odd coefficients, in z^2 */
            den = rs_tscale(exp, log, den, z2) ^ C[l];
            if (l == 1) break;
        }
        if (den == 0) return -1;
        val[e] = (uint8_t)rs_tscale(exp, log, rs_tdiv(exp, log, num, den), p);
        if (val[e] == 0) return -1;
    }
    for (unsigned e = 0; e < L; ++e) r[pos[e]] ^= val[e];
    return (int)L;
}

/* One codeword r[0 .. N), r[0] the highest coefficient, in place. Returns the
 * bytes corrected, or -1 when no codeword lies within t. */
static int decode_codeword(uint8_t *r, unsigned N, unsigned P, const uint8_t *exp, const uint8_t *log)
{
    uint8_t S[RS_MAX_PARITY];
    return syndromes(r, N, P, exp, log, S) ? correct_errors(r, N, P, S, exp, log) : 0;
}

/* The first attempt on a word with the syndromes S, not all zero, and 1 <= f <= P flagged positions
 * flag[0 .. f), ascending. Gamma = prod (1 - X_e x) over them; the Forney syndromes T = S Gamma mod x^P, of
 * which T_f .. T_(P-1) obey the recurrence of the error locator Lambda alone; Berlekamp-Massey on those, L <=
 * (P - f) / 2; Lambda's roots among the positions that are not flagged; Psi = Lambda Gamma, Omega = S Psi mod
 * x^(L + f), and Forney's value at each of the L + f places. S then obeys Psi's recurrence from L + f on, and
 * Psi has L + f distinct roots: the word the values leave has zero syndromes, L errors outside the flags, 2 L
 * + f <= P. Returns the bytes that changed, or -1 when there is no such word. */
static int correct_errata(uint8_t *r, unsigned N, unsigned P, const uint8_t *S, const unsigned *flag, unsigned f,
                          const uint8_t *exp, const uint8_t *log)
{
    uint8_t G[RS_MAX_PSI], T[RS_MAX_PARITY], C[LOCATOR_SIZE], Psi[RS_MAX_PSI], om[RS_MAX_ERRATA];
    uint8_t val[RS_MAX_ERRATA];
    unsigned pos[RS_MAX_ERRATA];
    memset(G, 0, sizeof(G));
    G[0] = 1;
    for (unsigned i = 0; i < f; ++i) {   /* times (1 - X x), X = alpha^(N - 1 - x) */
        const unsigned z = N - 1u - flag[i];
        for (unsigned l = i + 1; l > 0; --l) G[l] ^= (uint8_t)rs_tscale(exp, log, G[l - 1], z);
        pos[i] = flag[i];
    }
    for (unsigned k = 0; k < P; ++k) {
        unsigned v = 0;
        for (unsigned l = 0; l <= f && l <= k; ++l) v ^= rs_tmul(exp, log, G[l], S[k - l]);
        T[k] = (uint8_t)v;
    }
    const unsigned L = locator(T + f, P - f, exp, log, C);
    if (2 * L > P - f) return -1;
    unsigned found = 0, fi = 0;
    for (unsigned x = 0; x < N; ++x) {
        if (fi < f && flag[fi] == x) {   /* a flagged position is no candidate */
            ++fi;
            continue;
        }
        const unsigned z = (255u - (N - 1u - x)) % 255u;   /* X^-1 = alpha^z */
        unsigned v = C[L];
        for (unsigned l = L; l-- > 0;) v = rs_tscale(exp, log, v, z) ^ C[l];
        if (v == 0) {
            if (found == L) return -1;
            pos[f + found++] = x;
        }
    }
    if (found != L) return -1;
    const unsigned nu = L + f;
    for (unsigned i = 0; i <= nu; ++i) {
        unsigned v = 0;
        for (unsigned l = 0; l <= L && l <= i; ++l)
            if (i - l <= f) v ^= rs_tmul(exp, log, C[l], G[i - l]);
        Psi[i] = (uint8_t)v;
    }
    for (unsigned i = 0; i < nu; ++i) {
        unsigned v = 0;
        for (unsigned l = 0; l <= i; ++l) v ^= rs_tmul(exp, log, Psi[l], S[i - l]);
        om[i] = (uint8_t)v;
    }
    int changed = 0;
    for (unsigned e = 0; e < nu; ++e) {
        const unsigned p = N - 1u - pos[e], z = (255u - p) % 255u, z2 = (2u * z) % 255u;
        unsigned num = 0, den = 0;
        for (unsigned i = nu; i-- > 0;) num = rs_tscale(exp, log, num, z) ^ om[i];
        for (unsigned l = (nu & 1u) ? nu : nu - 1u;; l -= 2) {   /* the odd coefficients, in z^2 */
            den = rs_tscale(exp, log, den, z2) ^ Psi[l];
            if (l == 1) break;
        }
        if (den == 0) return -1;
        val[e] = (uint8_t)rs_tscale(exp, log, rs_tdiv(exp, log, num, den), p);
        if (val[e] == 0 && e >= f) return -1;   /* a flagged byte may have been right; an error is not */
        changed += val[e] != 0;
    }
    for (unsigned e = 0; e < nu; ++e) r[pos[e]] ^= val[e];
    return changed;
}

/* demod_rs_frame_decode (erase and erec NULL) and demod_rs_frame_decode_erasures */
static int frame_decode(uint8_t *row, size_t cap, int len_bytes, int crc, int fec, const uint64_t *erase,
                        demod_frame_rs_t *out, demod_frame_erase_t *erec)
{
    const size_t c = (size_t)frame_crc_bytes(crc), h = (size_t)len_bytes;
    if (!row || !out || c == 0 || (len_bytes != 1 && len_bytes != 2) || cap > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    if (!rs_mode_valid((unsigned)fec)) return DEMOD_BAD_ARG;
    const unsigned P = rs_parity((unsigned)fec);
    const long long max_len = frame_max_len((unsigned)cap, (unsigned)h, (unsigned)c, P);
    if (max_len < 0 || max_len > DEMOD_MAX_FRAME_PAYLOAD) return DEMOD_BAD_ARG;
    memset(out, 0, sizeof(*out));
    if (erec) memset(erec, 0, sizeof(*erec));
    unsigned len = row[0];
    if (h == 2) len = (len << 8) | row[1];
    if (len > (unsigned)max_len) {
        out->status = DEMOD_RS_BAD_LENGTH;
        return (int)h;
    }
    const unsigned n = (unsigned)(h + c) + len;
    if (!P) return (int)n;
    const unsigned D = rs_codewords(n, P);
    uint8_t exp[RS_EXP_SIZE], log[256], word[255];
    build_tables(exp, log);
    out->codewords = D;
    for (unsigned j = 0; j < D; ++j) {
        const unsigned kj = rs_message_bytes(n, D, j), N = kj + P;
        unsigned flag[RS_MAX_ERRATA], f = 0;
        for (unsigned x = 0; x < N; ++x) {
            word[x] = row[rs_symbol_offset(n, D, kj, j, x)];
            if (erase && rs_symbol_flagged(erase, n, D, kj, j, x)) {
                if (f < P) flag[f] = x;
                ++f;
            }
        }
        int e;
        if (f == 0) {
            e = decode_codeword(word, N, P, exp, log);
        } else {
            uint8_t S[RS_MAX_PARITY];
            erec->erased += f;
            if (!syndromes(word, N, P, exp, log, S)) continue;   /* clean: its own codeword under every rule */
            e = f <= P ? correct_errata(word, N, P, S, flag, f, exp, log) : -1;
            if (e >= 0) {
                ++erec->used;
            } else {
                ++erec->fallback;
                e = correct_errors(word, N, P, S, exp, log);
            }
        }
        if (e < 0) {
            ++out->failed;
            continue;
        }
        out->corrected += (uint32_t)e;
        if (e)
            for (unsigned x = 0; x < N; ++x) row[rs_symbol_offset(n, D, kj, j, x)] = word[x];
    }
    out->status = out->failed ? DEMOD_RS_FAILED : DEMOD_RS_OK;
    return (int)(n + D * P);
}

int demod_rs_frame_decode(uint8_t *row, size_t cap, int len_bytes, int crc, int fec, demod_frame_rs_t *out)
{
    return frame_decode(row, cap, len_bytes, crc, fec, NULL, out, NULL);
}

int demod_rs_frame_decode_erasures(uint8_t *row, size_t cap, int len_bytes, int crc, int fec,
                                   const uint64_t *erase, demod_frame_rs_t *out, demod_frame_erase_t *erec)
{
    if (!erec || ((uintptr_t)erase & 7) != 0 || !rs_parity((unsigned)fec)) return DEMOD_BAD_ARG;
    return frame_decode(row, cap, len_bytes, crc, fec, erase, out, erec);
}
