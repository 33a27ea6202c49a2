// frames_rs.hip — the Reed-Solomon outer code's device stage (include/demod.h
// "Reed-Solomon outer code", DESIGN.md §4.9 "Reed-Solomon outer code"): a pass
// over the rows a frame scan (packed rows) or the Viterbi decode (decoded rows)
// wrote, which corrects up to t = P / 2 wrong bytes in each codeword of each
// row, in place, before the check reads the rows. Groups, rows and the walk as
// frame_rows.h; every index below is bounded by the clamped count, max_len and
// the row width alone. One launch, no workspace, no atomics, no
// floating point; every output byte is a function of the inputs alone, the
// same as demod_rs_frame_decode's (demod_rs.c).
//
// One wave per row. The row's n' bytes go into the wave's own LDS slice by
// coalesced loads. Then, 64 / P codewords at a time (slot = lane / P, i = lane
// % P):
//
//  syndromes  S_i = r(alpha^i) by Horner over the codeword's symbols. The byte
//             is read from one LDS address per slot (a broadcast); the
//             multiplication by the lane's constant alpha^i is a GF(2)-linear
//             map held in eight registers (eight conditional XORs), not a
//             log/exp lookup: data-dependent LDS indices would conflict on
//             banks in the one loop that every byte of every row goes through.
//             A ballot of "a syndrome is not zero" ends a clean group of
//             codewords there: the common case costs little more than reading
//             each byte once.
//  dirty codewords only, one at a time with the whole wave (the log/exp tables
//  are built in the wave's LDS the first time one is met):
//  locator    Berlekamp-Massey with coefficient l of the locator and of its
//             predecessor in lane l; the discrepancy is a shuffle XOR
//             reduction, the shift by x^m a shuffle.
//  roots      lane l tests positions l, l + 64, .. of the codeword's own k_j +
//             P; a ballot counts them against the degree and ranks them.
//  values     Forney, one lane per error; the lane stores its corrected byte.
//
// A codeword is accepted under the same conditions as on the host: L <= t, L
// roots among its positions, no zero denominator or value.
//
// With a mask (ERASE, demod_frames_rs_erasures_async; include/demod.h "erasure
// decoding"): the row's mask words sit in the wave's LDS slice beside the row.
// The syndrome pass and its clean ballot are the same. A dirty codeword with 1
// <= f <= P flagged positions first goes, with the whole wave, through
//  flags      the flagged positions of the codeword, ranked by ballot
//  Gamma      the erasure locator, coefficient l in lane l: one shuffle and one
//             table multiply per erasure
//  Forney     lane k forms syndrome k of S Gamma mod x^P; the same
//  syndromes  Berlekamp-Massey runs on the last P - f of them, L <= (P - f) / 2
//  roots      as above, skipping flagged positions
//  values     Psi = Lambda Gamma and Omega = S Psi mod x^(L + f), coefficient l
//             by lane l; Forney, one lane per erratum, up to P lanes. A zero
//             value is allowed at a flagged position alone.
// and on "nothing found" (or f > P) through rs_correct on the same syndromes.
#include <type_traits>

#include "frame_rows.h"
#include "rs_ops.h"

namespace fskd {

// n' at the payload limit is 4710 (h = 2, c = 4, P = 32, D = 19), rounded up to a multiple of 8
constexpr unsigned kRsRowBytes = 4712;
static_assert(2 + DEMOD_MAX_FRAME_PAYLOAD + 4 + 19 * 32 <= kRsRowBytes, "the longest protected frame");

struct RsWaveLds {
    uint8_t row[kRsRowBytes];
    uint8_t exp[512];                 // RS_EXP_SIZE entries
    uint8_t log[256];
    uint8_t syn[RS_MAX_PARITY];
    uint8_t lam[RS_MAX_T + 4];        // the locator's coefficients 0 .. t
    uint8_t om[RS_MAX_T];
    uint8_t pos[RS_MAX_T];
};

// what the first attempt of a codeword with flags adds: under 1 KB a wave
struct RsWaveLdsErase : RsWaveLds {
    uint64_t mask[(kRsRowBytes + 63) / 64];   // the row's mask words
    uint8_t gam[RS_MAX_PSI + 3];      // Gamma's coefficients 0 .. f
    uint8_t fsyn[RS_MAX_PARITY];      // the Forney syndromes
    uint8_t elam[RS_MAX_T + 4];       // Lambda's coefficients 0 .. L
    uint8_t psi[RS_MAX_PSI + 3];      // Psi's coefficients 0 .. L + f
    uint8_t eom[RS_MAX_ERRATA];
    uint8_t epos[RS_MAX_ERRATA];      // the flagged positions, then Lambda's roots
};

static __device__ __forceinline__ unsigned rs_uniform(unsigned v)
{
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

static __device__ __forceinline__ unsigned rs_wave_xor(unsigned v)
{
    for (int d = 32; d > 0; d >>= 1) v ^= (unsigned)__shfl_xor((int)v, d);
    return v;
}

// exp and log of the wave, 64 lanes: entry e = lane + 64 q
static __device__ __forceinline__ void rs_wave_tables(RsWaveLds &w, int lane)
{
    unsigned c64 = 1, v = 1;
    for (int k = 0; k < 64; ++k) c64 = rs_xtime(c64);
    for (int k = 0; k < lane; ++k) v = rs_xtime(v);
    if (lane == 0) w.log[0] = 0;
    for (unsigned e = (unsigned)lane; e < 255u; e += 64u) {
        rs_table_entry(e, v, w.exp, w.log);
        v = rs_mul(v, c64);
    }
}

// Berlekamp-Massey on syn[0 .. count), count <= P: lane l holds coefficient l of C (the locator) and of B.
// Returns the lane's coefficient; L the locator's length. The whole wave.
static __device__ __forceinline__ unsigned rs_locator(RsWaveLds &w, const uint8_t *syn, const unsigned count,
                                                      int lane, unsigned &Lout)
{
    const unsigned l = (unsigned)lane;
    unsigned C = l == 0 ? 1u : 0u, B = C;
    unsigned L = 0, m = 1, b = 1;
    for (unsigned k = 0; k < count; ++k) {
        const unsigned term = (l <= L && l <= k) ? rs_tmul(w.exp, w.log, C, syn[k - l]) : 0u;
        const unsigned d = rs_uniform(rs_wave_xor(term));
        const unsigned Bs = (unsigned)__shfl((int)B, l >= m ? (int)(l - m) : lane);
        if (d == 0) {
            ++m;
            continue;
        }
        const unsigned coef = rs_tdiv(w.exp, w.log, d, b);
        const unsigned T = C;
        if (l >= m) C ^= rs_tmul(w.exp, w.log, coef, Bs);
        if (2 * L <= k) {
            L = k + 1 - L;
            B = T;
            b = d;
            m = 1;
        } else {
            ++m;
        }
    }
    Lout = L;
    return C;
}

// One dirty codeword j of a frame of n bytes in D codewords, its syndromes in
// w.syn; the whole wave. Returns the bytes corrected (stored to grow), or -1.
// Wave-uniform: every branch below is on a value all lanes share.
template <int P>
static __device__ __forceinline__ int rs_correct(RsWaveLds &w, uint8_t *grow, unsigned n, unsigned D, unsigned j,
                                                 unsigned kj, int lane)
{
    constexpr unsigned kT = P / 2;
    const unsigned N = kj + P, l = (unsigned)lane;
    unsigned L;
    const unsigned C = rs_locator(w, w.syn, (unsigned)P, lane, L);
    if (L > kT) return -1;
    wave_sync();   // the codeword before has read lam, om and pos
    if (l <= kT) w.lam[l] = (uint8_t)C;
    wave_sync();
    // the roots among the codeword's own positions: x has X = alpha^(N - 1 - x)
    unsigned found = 0;
    for (unsigned x0 = 0; x0 < N; x0 += kRowLanes) {
        const unsigned x = x0 + l;
        bool root = false;
        if (x < N) {
            const unsigned z = (255u - (N - 1u - x)) % 255u;
            unsigned v = w.lam[L];
            for (unsigned i = L; i-- > 0;) v = rs_tscale(w.exp, w.log, v, z) ^ w.lam[i];
            root = v == 0;
        }
        const unsigned long long bal = __ballot(root);
        const unsigned rank = found + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        if (root && rank < kT) w.pos[rank] = (uint8_t)x;
        found += (unsigned)__popcll(bal);
    }
    if (found != L) return -1;
    // Forney: omega = S(x) C(x) mod x^L, e = X omega(X^-1) / C'(X^-1)
    if (l < L) {
        unsigned v = 0;
        for (unsigned i = 0; i <= l; ++i) v ^= rs_tmul(w.exp, w.log, w.lam[i], w.syn[l - i]);
        w.om[l] = (uint8_t)v;
    }
    wave_sync();
    unsigned val = 0, at = 0;
    bool bad = false;
    if (l < L) {
        const unsigned x = w.pos[l], p = N - 1u - x, z = (255u - p) % 255u, z2 = (2u * z) % 255u;
        unsigned num = 0, den = 0;
        for (unsigned i = L; i-- > 0;) num = rs_tscale(w.exp, w.log, num, z) ^ w.om[i];
        for (unsigned i = (L & 1u) ? L : L - 1u;; i -= 2) {   // the odd coefficients, in z^2
            den = rs_tscale(w.exp, w.log, den, z2) ^ w.lam[i];
            if (i == 1) break;
        }
        if (den != 0) val = rs_tscale(w.exp, w.log, rs_tdiv(w.exp, w.log, num, den), p);
        bad = val == 0;
        at = rs_symbol_offset(n, D, kj, j, x);   // x < N: inside the frame's n' bytes
    }
    if (__ballot(bad)) return -1;
    if (l < L) grow[at] = (uint8_t)(w.row[at] ^ val);
    return (int)L;
}

// The first attempt on one dirty codeword (include/demod.h "erasure decoding"), its syndromes in w.syn and
// the row's mask in w.mask; the whole wave. f: its flagged positions. Returns the bytes that changed (stored
// to grow), or -1 when it found nothing (f == 0 and f > P included): w.syn is as it was. Wave-uniform.
template <int P>
static __device__ __forceinline__ int rs_correct_errata(RsWaveLdsErase &w, uint8_t *grow, unsigned n, unsigned D,
                                                        unsigned j, unsigned kj, int lane, unsigned &f)
{
    const unsigned N = kj + P, l = (unsigned)lane;
    const unsigned long long below = (1ull << lane) - 1ull;
    wave_sync();   // the codeword before has read the lists below
    f = 0;
    for (unsigned x0 = 0; x0 < N; x0 += kRowLanes) {
        const unsigned x = x0 + l;
        const bool flag = x < N && rs_symbol_flagged(w.mask, n, D, kj, j, x);
        const unsigned long long bal = __ballot(flag);
        const unsigned rank = f + (unsigned)__popcll(bal & below);
        if (flag && rank < (unsigned)P) w.epos[rank] = (uint8_t)x;
        f += (unsigned)__popcll(bal);
    }
    if (f == 0 || f > (unsigned)P) return -1;
    wave_sync();
    // Gamma = prod (1 - X x) over the flags, X = alpha^(N - 1 - x): coefficient l in lane l
    unsigned G = l == 0 ? 1u : 0u;
    for (unsigned i = 0; i < f; ++i) {
        const unsigned z = N - 1u - w.epos[i];
        const unsigned Gs = (unsigned)__shfl((int)G, l ? lane - 1 : 0);
        if (l) G ^= rs_tscale(w.exp, w.log, Gs, z);
    }
    if (l <= f) w.gam[l] = (uint8_t)G;
    wave_sync();
    if (l < (unsigned)P) {   // Forney syndrome l of S Gamma mod x^P
        unsigned v = 0;
        for (unsigned i = 0; i <= f && i <= l; ++i) v ^= rs_tmul(w.exp, w.log, w.gam[i], w.syn[l - i]);
        w.fsyn[l] = (uint8_t)v;
    }
    wave_sync();
    unsigned L;
    const unsigned C = rs_locator(w, w.fsyn + f, (unsigned)P - f, lane, L);
    if (2u * L > (unsigned)P - f) return -1;
    if (l <= L) w.elam[l] = (uint8_t)C;
    wave_sync();
    // Lambda's roots among the codeword's own positions that are not flagged
    unsigned found = 0;
    for (unsigned x0 = 0; x0 < N; x0 += kRowLanes) {
        const unsigned x = x0 + l;
        bool root = false;
        if (x < N && !rs_symbol_flagged(w.mask, n, D, kj, j, x)) {
            const unsigned z = (255u - (N - 1u - x)) % 255u;
            unsigned v = w.elam[L];
            for (unsigned i = L; i-- > 0;) v = rs_tscale(w.exp, w.log, v, z) ^ w.elam[i];
            root = v == 0;
        }
        const unsigned long long bal = __ballot(root);
        const unsigned rank = found + (unsigned)__popcll(bal & below);
        if (root && rank < L) w.epos[f + rank] = (uint8_t)x;   // f + L <= P
        found += (unsigned)__popcll(bal);
    }
    if (found != L) return -1;
    const unsigned nu = L + f;
    if (l <= nu) {   // Psi = Lambda Gamma
        unsigned v = 0;
        for (unsigned i = 0; i <= L && i <= l; ++i)
            if (l - i <= f) v ^= rs_tmul(w.exp, w.log, w.elam[i], w.gam[l - i]);
        w.psi[l] = (uint8_t)v;
    }
    wave_sync();
    if (l < nu) {   // Omega = S Psi mod x^nu
        unsigned v = 0;
        for (unsigned i = 0; i <= l; ++i) v ^= rs_tmul(w.exp, w.log, w.psi[i], w.syn[l - i]);
        w.eom[l] = (uint8_t)v;
    }
    wave_sync();
    unsigned val = 0, at = 0;
    bool bad = false;
    if (l < nu) {   // Forney, a lane an erratum: e = X Omega(X^-1) / Psi'(X^-1)
        const unsigned x = w.epos[l], p = N - 1u - x, z = (255u - p) % 255u, z2 = (2u * z) % 255u;
        unsigned num = 0, den = 0;
        for (unsigned i = nu; i-- > 0;) num = rs_tscale(w.exp, w.log, num, z) ^ w.eom[i];
        for (unsigned i = (nu & 1u) ? nu : nu - 1u;; i -= 2) {   // the odd coefficients, in z^2
            den = rs_tscale(w.exp, w.log, den, z2) ^ w.psi[i];
            if (i == 1) break;
        }
        if (den != 0) val = rs_tscale(w.exp, w.log, rs_tdiv(w.exp, w.log, num, den), p);
        bad = den == 0 || (val == 0 && l >= f);   // a flagged byte may have been right; an error is not
        at = rs_symbol_offset(n, D, kj, j, x);    // x < N: inside the frame's n' bytes
    }
    if (__ballot(bad)) return -1;
    const bool change = l < nu && val != 0;
    if (change) grow[at] = (uint8_t)(w.row[at] ^ val);
    return (int)__popcll(__ballot(change));
}

template <int P, bool ERASE>
__global__ __launch_bounds__(kRowThreads) void frames_rs_kernel(
    typename std::conditional<ERASE, FramesRsEraseParams, FramesRsParams>::type p, unsigned wpg)
{
    using Lds = typename std::conditional<ERASE, RsWaveLdsErase, RsWaveLds>::type;
    __shared__ Lds s_w[kRowWaves];
    constexpr unsigned kSlots = kRowLanes / P;
    const int wave = threadIdx.x / kRowLanes, lane = threadIdx.x % kRowLanes;
    const RowWave rw = row_wave(p.n_groups, wpg);
    if (!rw.live) return;
    const unsigned g = rw.g;
    const unsigned nw = rows_clamped(p.res[g].n_written, p.max_frames);
    Lds &w = s_w[wave];   // the wave's own LDS slice: no other wave touches it
    const unsigned slot = (unsigned)lane / P, si = (unsigned)lane % P;
    // times alpha^si as a GF(2)-linear map: col[b] = alpha^(si + b)
    unsigned col[8], asi = 1;
    for (unsigned k = 0; k < si; ++k) asi = rs_xtime(asi);
    rs_times_cols(col, asi);
    const unsigned h = (unsigned)p.len_bytes;
    bool tables = false;
    for (unsigned i = rw.c; i < nw; i += wpg) {   // the same for every lane of the wave
        const size_t r = (size_t)g * p.max_frames + i;
        uint8_t *grow = p.rows + r * p.row_bytes;
        const unsigned len = row_length_load(grow, h);
        demod_frame_rs_t out;
        out.status = DEMOD_RS_BAD_LENGTH;
        out.codewords = out.corrected = out.failed = 0;
        demod_frame_erase_t er;
        er.erased = er.used = er.fallback = er.reserved = 0;
        const unsigned n = h + len + (unsigned)p.crc_bytes;
        const unsigned D = rs_codewords(n, P), np = n + D * P;
        // len <= max_len gives n' <= row_bytes and <= kRsRowBytes (the host checked max_len)
        if (len <= p.max_len && np <= p.row_bytes && np <= kRsRowBytes) {
            wave_sync();   // the row before has been read
            for (unsigned b = (unsigned)lane; b < np; b += kRowLanes) w.row[b] = grow[b];
            if constexpr (ERASE) {   // the words that hold the frame's n' <= row_bytes bytes; the bits past n' off
                const unsigned Wm = rs_mask_words(p.row_bytes);
                unsigned cnt = 0;
                for (unsigned wd = (unsigned)lane; wd * 64u < np; wd += kRowLanes) {
                    uint64_t m = p.erase[r * Wm + wd];
                    if (np - wd * 64u < 64u) m &= ((uint64_t)1 << (np - wd * 64u)) - 1u;
                    w.mask[wd] = m;
                    cnt += (unsigned)__popcll(m);
                }
                for (int d = 32; d > 0; d >>= 1) cnt += (unsigned)__shfl_xor((int)cnt, d);
                er.erased = cnt;
            }
            wave_sync();
            unsigned corrected = 0, failed = 0;
            for (unsigned j0 = 0; j0 < D; j0 += kSlots) {
                const unsigned j = j0 + slot;
                const bool have = j < D;
                const unsigned kj = have ? rs_message_bytes(n, D, j) : 1u, N = kj + P;
                const unsigned Nmost = rs_message_bytes(n, D, j0) + P;   // k_j does not grow with j
                unsigned syn = 0, off = j;
                // The trip count is the wave's (Nmost); a slot with a shorter codeword, or none, sits
                // out its last steps. The branch holds one LDS read and lane-local arithmetic: no
                // shuffle, ballot or barrier inside it.
                for (unsigned x = 0; x < Nmost; ++x) {
                    if (have && x < N) {
                        const unsigned s = syn;
                        unsigned v = w.row[off];
#pragma unroll
                        for (int b = 0; b < 8; ++b) v ^= ((s >> b) & 1u) ? col[b] : 0u;
                        syn = v;
                        off = x + 1u == kj ? n + j : off + D;
                    }
                }
                const unsigned long long dirty = __ballot(have && syn != 0);
                if (!dirty) continue;
                if (!tables) {
                    rs_wave_tables(w, lane);
                    tables = true;
                }
                for (unsigned s = 0; s < kSlots; ++s) {
                    const unsigned long long mask = (P == 64 ? ~0ull : (1ull << P) - 1ull) << (s * P);
                    if (!(dirty & mask)) continue;
                    wave_sync();   // the codeword before has read syn
                    if (slot == s) w.syn[si] = (uint8_t)syn;
                    wave_sync();
                    const unsigned js = j0 + s;
                    int e = -1;
                    if constexpr (ERASE) {
                        unsigned f;
                        e = rs_correct_errata<P>(w, grow, n, D, js, rs_message_bytes(n, D, js), lane, f);
                        if (e >= 0) ++er.used;
                        else if (f) ++er.fallback;
                    }
                    if (e < 0) e = rs_correct<P>(w, grow, n, D, js, rs_message_bytes(n, D, js), lane);
                    if (e < 0) ++failed;
                    else corrected += (unsigned)e;
                }
            }
            out.status = failed ? DEMOD_RS_FAILED : DEMOD_RS_OK;
            out.codewords = D;
            out.corrected = corrected;
            out.failed = failed;
        }
        if (lane == 0) p.rs[r] = out;
        if constexpr (ERASE)
            if (lane == 0) p.erec[r] = er;
    }
}

hipError_t launch_frames_rs(const FramesRsParams &p, hipStream_t s)
{
    const unsigned wpg = row_waves_per_group(p.n_groups, p.max_frames), blocks = row_blocks(p.n_groups, wpg);
    if (p.parity == 16)
        hipLaunchKernelGGL((frames_rs_kernel<16, false>), dim3(blocks), dim3(kRowThreads), 0, s, p, wpg);
    else
        hipLaunchKernelGGL((frames_rs_kernel<32, false>), dim3(blocks), dim3(kRowThreads), 0, s, p, wpg);
    return hipGetLastError();
}

hipError_t launch_frames_rs_erasures(const FramesRsEraseParams &p, hipStream_t s)
{
    const unsigned wpg = row_waves_per_group(p.n_groups, p.max_frames), blocks = row_blocks(p.n_groups, wpg);
    if (p.parity == 16)
        hipLaunchKernelGGL((frames_rs_kernel<16, true>), dim3(blocks), dim3(kRowThreads), 0, s, p, wpg);
    else
        hipLaunchKernelGGL((frames_rs_kernel<32, true>), dim3(blocks), dim3(kRowThreads), 0, s, p, wpg);
    return hipGetLastError();
}

}  // namespace fskd
