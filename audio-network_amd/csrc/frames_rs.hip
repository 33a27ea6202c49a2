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

// One dirty codeword j of a frame of n bytes in D codewords, its syndromes in
// w.syn; the whole wave. Returns the bytes corrected (stored to grow), or -1.
// Wave-uniform: every branch below is on a value all lanes share.
template <int P>
static __device__ __forceinline__ int rs_correct(RsWaveLds &w, uint8_t *grow, unsigned n, unsigned D, unsigned j,
                                                 unsigned kj, int lane)
{
    constexpr unsigned kT = P / 2;
    const unsigned N = kj + P, l = (unsigned)lane;
    // Berlekamp-Massey: lane l holds coefficient l of C (the locator) and of B
    unsigned C = l == 0 ? 1u : 0u, B = C;
    unsigned L = 0, m = 1, b = 1;
    for (unsigned k = 0; k < (unsigned)P; ++k) {
        const unsigned term = (l <= L && l <= k) ? rs_tmul(w.exp, w.log, C, w.syn[k - l]) : 0u;
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

template <int P>
__global__ __launch_bounds__(kRowThreads) void frames_rs_kernel(FramesRsParams p, unsigned wpg)
{
    __shared__ RsWaveLds s_w[kRowWaves];
    constexpr unsigned kSlots = kRowLanes / P;
    const int wave = threadIdx.x / kRowLanes, lane = threadIdx.x % kRowLanes;
    const RowWave rw = row_wave(p.n_groups, wpg);
    if (!rw.live) return;
    const unsigned g = rw.g;
    const unsigned nw = rows_clamped(p.res[g].n_written, p.max_frames);
    RsWaveLds &w = s_w[wave];   // the wave's own LDS slice: no other wave touches it
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
        const unsigned n = h + len + (unsigned)p.crc_bytes;
        const unsigned D = rs_codewords(n, P), np = n + D * P;
        // len <= max_len gives n' <= row_bytes and <= kRsRowBytes (the host checked max_len)
        if (len <= p.max_len && np <= p.row_bytes && np <= kRsRowBytes) {
            wave_sync();   // the row before has been read
            for (unsigned b = (unsigned)lane; b < np; b += kRowLanes) w.row[b] = grow[b];
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
                    const int e = rs_correct<P>(w, grow, n, D, js, rs_message_bytes(n, D, js), lane);
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
    }
}

hipError_t launch_frames_rs(const FramesRsParams &p, hipStream_t s)
{
    const unsigned wpg = row_waves_per_group(p.n_groups, p.max_frames), blocks = row_blocks(p.n_groups, wpg);
    if (p.parity == 16)
        hipLaunchKernelGGL(frames_rs_kernel<16>, dim3(blocks), dim3(kRowThreads), 0, s, p, wpg);
    else
        hipLaunchKernelGGL(frames_rs_kernel<32>, dim3(blocks), dim3(kRowThreads), 0, s, p, wpg);
    return hipGetLastError();
}

}  // namespace fskd
