// frames_tx.hip — the transmitter's device stages (include/demod.h
// "transmitter", DESIGN.md §4.9 "Transmitter"): frames to queued symbols
// (encode: plan, write) and queued symbols to samples (modulate: phase,
// samples, state). Per stream the state {head, tail, offset, phase, counters}
// and a [C] byte ring of symbols at q mod C live on the device. Every launch
// clamps what it reads of the state (offset <= n - 1, head + (offset > 0) <=
// tail <= head + C) and every count against its bound, and every ring index is
// taken mod C: no content of the state, the tables, the ring or the workspace
// moves an access outside the arrays. No atomics, no floating point; every
// output byte is a function of the inputs alone. Five launches in all, whatever
// the counts are:
//
//  plan     one wave per stream walks its records 64 at a time: a_i = A(len_i)
//           + gap (0 for a length above max_len), the inclusive prefix e by a
//           shuffle scan with a running carry, acceptance tail + e - head <= C,
//           the places; then tail, accepted, refused.
//  write    one wave per frame (frame_rows.h's walk, a stream's records its
//           rows). len || data || CRC in the wave's LDS, the CRC by the
//           check's lane-split scheme (crc_ops.h); with an outer
//           code (rs_ops.h) its parity behind them, 64 / P codewords at a time:
//           lane (slot, i) holds byte i of the slot's parity register, a step
//           takes the register's top byte and the neighbour's by shuffle, and
//           the product with the lane's generator coefficient is a GF(2)-linear
//           map in eight registers. Then lane j
//           writes symbols j, j + 64, ..: the word, the payload symbols, the
//           gap's idle symbols. An air bit goes back through the mode's map
//           (fec_map.h) to its mother bit m, which reads the information bits
//           (m >> 1) - 6 .. m >> 1 alone: the encoder has no serial step.
//  phase    one workgroup per stream, 1 to 16 waves by the symbols a pull can
//           touch: PHI of every symbol, a two-level uint32 prefix sum of n
//           inc[sym(q)]: each thread sums 4 consecutive symbols, a shuffle scan
//           joins a wave, the waves' totals meet in LDS, a running carry joins
//           the steps. work[s][d] = PHI(head + d) for d >= 1; PHI(head) is the
//           state's phase, and slot 0 holds head mod C, so that no other
//           thread divides a 64-bit index.
//  samples  one thread per 8 samples, one 16-byte store; the last samples of a
//           run whose count is not a multiple of 8 take 2-byte stores. The 8
//           samples touch at most two symbols.
//  state    one thread per stream; last, as the other two read the state. A
//           pull that ends inside an idle symbol past the queue stores that
//           symbol in the ring: it is queued now (tail' = head' + 1), and the
//           next pull reads it there.
#include "crc_ops.h"
#include "frame_rows.h"
#include "synth_ops.h"

namespace fskd {

constexpr int kTxPhaseRun = 4;        // phase: consecutive symbols a thread sums per step
constexpr int kTxPhaseMaxWaves = 16;  // phase: waves a stream at most (one workgroup)
// len || data || CRC || parity of the longest frame (19 codewords of 32 parity
// bytes), rounded up to a multiple of 8
constexpr int kTxFrameBytes = (2 + DEMOD_MAX_FRAME_PAYLOAD + 4 + 19 * RS_MAX_PARITY + 7) / 8 * 8;

// symbol i < 64 of a pattern packed 16 symbols to a word
static __device__ __forceinline__ unsigned tx_sym4(const unsigned long long (&w)[4], unsigned i)
{
    unsigned long long v = w[0];
    if ((i >> 4) == 1) v = w[1];
    if ((i >> 4) == 2) v = w[2];
    if ((i >> 4) == 3) v = w[3];
    return (unsigned)(v >> ((i & 15u) * 4u)) & 15u;
}

static __device__ __forceinline__ uint32_t tx_inc(const TxParams &p, unsigned sym)
{
    uint32_t inc = 0;
#pragma unroll
    for (int t = 0; t < kMaxTones; ++t)
        if ((unsigned)t == sym) inc = p.inc[t];
    return inc;
}

struct TxState {
    unsigned long long head, tail;
    unsigned offset, phase;
};

// the stream's state, clamped into its invariant
static __device__ __forceinline__ TxState tx_load(const TxParams &p, unsigned s)
{
    const demod_tx_stream_state_t *st = p.state + s;
    TxState t;
    t.head = st->head;
    t.tail = st->tail;
    t.offset = st->offset < p.n - 1 ? st->offset : p.n - 1;
    t.phase = st->phase;
    const unsigned long long lo = t.head + (t.offset > 0 ? 1u : 0u), hi = t.head + p.ring_symbols;
    if (t.tail > hi) t.tail = hi;
    if (t.tail < lo) t.tail = lo;
    return t;
}

// Sp(len): the payload symbols of a frame of len data bytes, frame_shape.h's
// span (kept: Nt(T), the frame's code bits, 0 without a code)
static __device__ __forceinline__ unsigned tx_payload_symbols(const TxParams &p, unsigned len, unsigned &kept)
{
    unsigned T;
    return frame_air_symbols(len, (unsigned)p.len_bytes, (unsigned)p.crc_bytes, (unsigned)p.bits, (unsigned)p.fec,
                             (unsigned)p.parity, &T, &kept);
}

__global__ __launch_bounds__(kRowThreads) void tx_plan_kernel(TxParams p)
{
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const unsigned long long s64 = (unsigned long long)blockIdx.x * kRowWaves + wave;
    if (s64 >= p.n_streams) return;
    const unsigned s = (unsigned)s64;
    const TxState t = tx_load(p, s);
    const unsigned cnt = rows_clamped(p.count[s], p.max_frames);
    const size_t row0 = (size_t)s * p.max_frames;
    const unsigned long long used = t.tail - t.head, C = p.ring_symbols;
    unsigned long long carry = 0, last_e = 0;
    unsigned n_acc = 0;
    for (unsigned base = 0; base < cnt; base += 64) {   // the same for every lane of the wave
        const unsigned i = base + (unsigned)lane;
        const bool in = i < cnt;
        const unsigned len = in ? p.records[row0 + i].length : 0u;
        const bool valid = in && len <= p.max_len;
        unsigned kept, A = 0;
        if (valid) A = p.sync_len + tx_payload_symbols(p, len, kept);
        const unsigned long long a = valid ? (unsigned long long)A + p.gap : 0ull;
        unsigned long long x = a;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        const unsigned long long e = carry + x;
        const bool ok = valid && used + e <= C;
        if (in) {
            demod_tx_place_t pl;
            pl.start = ok ? t.tail + e - a : 0ull;
            pl.symbols = ok ? A : 0u;
            pl.status = ok ? DEMOD_TX_OK : valid ? DEMOD_TX_NO_ROOM : DEMOD_TX_BAD_LENGTH;
            p.place[row0 + i] = pl;
        }
        const unsigned long long okb = __ballot(ok);
        if (okb) last_e = __shfl(e, 63 - __clzll((long long)okb));
        n_acc += (unsigned)__popcll(okb);
        carry = __shfl(e, 63);
    }
    if (lane == 0) {
        demod_tx_stream_state_t *st = p.state + s;
        const unsigned long long acc = st->accepted, ref = st->refused;
        st->head = t.head;
        st->tail = t.tail + last_e;
        st->accepted = acc + n_acc;
        st->refused = ref + (cnt - n_acc);
        st->offset = t.offset;
        st->phase = t.phase;
    }
}

template <int WIDTH>
__global__ __launch_bounds__(kRowThreads) void tx_write_kernel(TxParams p, unsigned wpg)
{
    __shared__ unsigned s_tab[256];
    __shared__ uint8_t s_frame[kRowWaves][kTxFrameBytes];
    const int wave = threadIdx.x / kRowLanes, lane = threadIdx.x % kRowLanes;
    crc_byte_table(s_tab, p.poly);
    __syncthreads();
    const RowWave rw = row_wave(p.n_streams, wpg);
    if (!rw.live) return;
    const unsigned g = rw.g;
    const unsigned cnt = rows_clamped(p.count[g], p.max_frames);
    const unsigned h = (unsigned)p.len_bytes, cb = (unsigned)p.crc_bytes, bits = (unsigned)p.bits;
    const unsigned C = p.ring_symbols, L = p.sync_len;
    uint8_t *buf = s_frame[wave];
    uint8_t *ring = p.ring + (size_t)g * C;
    // the outer code: lane (slot, si) of 64 / P slots; times the lane's generator
    // coefficient g[si + 1] as a GF(2)-linear map, col[b] = g[si + 1] alpha^b
    const unsigned P = (unsigned)p.parity;   // 0, 16 or 32
    const unsigned slot = P == 16 ? (unsigned)lane >> 4 : (unsigned)lane >> 5, si = P ? (unsigned)lane & (P - 1u) : 0u;
    unsigned col[8];
    {
        unsigned long long w = p.rs_g8[0];
        if ((si >> 3) == 1) w = p.rs_g8[1];
        if ((si >> 3) == 2) w = p.rs_g8[2];
        if ((si >> 3) == 3) w = p.rs_g8[3];
        rs_times_cols(col, (unsigned)(w >> ((si & 7u) * 8u)) & 0xFFu);
    }
    for (unsigned i = rw.c; i < cnt; i += wpg) {   // the same for every lane of the wave
        const size_t r = (size_t)g * p.max_frames + i;
        const demod_tx_place_t pl = p.place[r];   // plan's, of this call
        if (pl.status != DEMOD_TX_OK) continue;
        const unsigned len = p.records[r].length < p.max_len ? p.records[r].length : p.max_len;
        const unsigned lenc = len < p.n_bytes ? len : p.n_bytes;
        const unsigned off = p.records[r].body < p.n_bytes - lenc ? p.records[r].body : p.n_bytes - lenc;
        wave_sync();   // the wave's own LDS row: the frame before has been read
        row_length_store(buf, h, len, lane);
        for (unsigned b = (unsigned)lane; b < len; b += 64)
            buf[h + b] = b < lenc ? p.bytes[off + b] : (uint8_t)0;
        wave_sync();
        const unsigned n = h + len;
        unsigned nb = n + cb;
        const unsigned crc = crc_wave<WIDTH>(buf, n, lane, p.init, p.poly, p.xpow8, s_tab) >> (32 - WIDTH);
        if (lane < (int)cb) buf[n + lane] = (uint8_t)(crc >> (8 * (cb - 1 - (unsigned)lane)));
        wave_sync();
        if (P) {
            const unsigned n0 = nb, D = rs_codewords(n0, P);
            for (unsigned j0 = 0; j0 < D; j0 += 64u / P) {   // the same for every lane of the wave
                const unsigned j = j0 + slot;
                const bool have = j < D;
                const unsigned kj = have ? rs_message_bytes(n0, D, j) : 0u;
                const unsigned kmost = rs_message_bytes(n0, D, j0);   // k_j does not grow with j
                unsigned par = 0, at = j;
                for (unsigned x = 0; x < kmost; ++x) {
                    // the register's top byte (the slot's lane 0) and the byte below this lane's
                    const unsigned top = (unsigned)__shfl((int)par, (int)(slot * P));
                    const unsigned below = (unsigned)__shfl((int)par, lane < 63 ? lane + 1 : lane);
                    if (have && x < kj) {
                        const unsigned f = buf[at] ^ top;
                        unsigned v = si + 1u < P ? below : 0u;
#pragma unroll
                        for (int b = 0; b < 8; ++b) v ^= ((f >> b) & 1u) ? col[b] : 0u;
                        par = v;
                        at += D;
                    }
                }
                if (have) buf[n0 + si * D + j] = (uint8_t)par;   // parity byte si D + j
            }
            nb = n0 + D * P;   // n' <= kTxFrameBytes: len <= max_len <= DEMOD_MAX_FRAME_PAYLOAD
            wave_sync();
        }
        unsigned kept;
        const unsigned A = L + tx_payload_symbols(p, len, kept);
        const unsigned total = A + p.gap;            // <= C
        const unsigned sm = (unsigned)(pl.start % C);
        const unsigned long long i0 = pl.start % p.idle_len;
        for (unsigned j = (unsigned)lane; j < total; j += 64) {
            unsigned sym;
            if (j < L) {
                sym = tx_sym4(p.sync4, j);
            } else if (j >= A) {
                sym = tx_sym4(p.idle4, (unsigned)((i0 + j) % p.idle_len));
            } else if (!p.fec) {
                // bits [bp, bp + bits) of the frame's bytes, MSB first; past the end 0
                const unsigned bp = (j - L) * bits, B0 = bp >> 3;
                const unsigned w = ((B0 < nb ? buf[B0] : 0u) << 8) | (B0 + 1 < nb ? buf[B0 + 1] : 0u);
                sym = (w >> (16 - (bp & 7u) - bits)) & ((1u << bits) - 1u);
            } else {
                sym = 0;
                for (unsigned b = 0; b < bits; ++b) {
                    // air bit a -> code index (the interleaver is its own inverse) -> mother bit
                    const unsigned ci = fec_interleave((unsigned)p.fec, (j - L) * bits + b);
                    unsigned v = 0;
                    if (ci < kept) {   // else a pad position of the last block or symbol
                        const unsigned m = fec_mother_bit((unsigned)p.fec, ci);
                        // the register after step m >> 1: information bits lo .. lo + 6, the newest lowest
                        const int lo = (int)(m >> 1) - 6, B0 = lo >> 3;
                        const unsigned w = ((B0 >= 0 && (unsigned)B0 < nb ? buf[B0] : 0u) << 8) |
                                           (B0 + 1 >= 0 && (unsigned)(B0 + 1) < nb ? buf[B0 + 1] : 0u);
                        const unsigned reg = (w >> (9 - (unsigned)(lo - 8 * B0))) & 0x7Fu;
                        v = (unsigned)__popc(reg & ((m & 1u) ? 0133u : 0171u)) & 1u;
                    }
                    sym = (sym << 1) | v;
                }
            }
            const unsigned at = sm + j;   // < 2 C
            ring[at >= C ? at - C : at] = (uint8_t)sym;
        }
    }
}

hipError_t launch_tx_encode(const TxParams &p, hipStream_t s)
{
    const unsigned S = p.n_streams;
    hipLaunchKernelGGL(tx_plan_kernel, dim3((S + kRowWaves - 1) / kRowWaves), dim3(kRowThreads), 0, s, p);
    const unsigned wpg = row_waves_per_group(S, p.max_frames), blocks = row_blocks(S, wpg);
    if (p.crc_bytes == 2)
        hipLaunchKernelGGL(tx_write_kernel<16>, dim3(blocks), dim3(kRowThreads), 0, s, p, wpg);
    else
        hipLaunchKernelGGL(tx_write_kernel<32>, dim3(blocks), dim3(kRowThreads), 0, s, p, wpg);
    return hipGetLastError();
}

// sym(head + d) for the stream whose head mod C is hm
static __device__ __forceinline__ unsigned tx_symbol(const TxParams &p, const TxState &t, const uint8_t *ring,
                                                     unsigned hm, unsigned d)
{
    const unsigned long long q = t.head + d;
    if (q < t.tail) return ring[(hm + d) % p.ring_symbols] & 15u;   // hm + d < 2^32
    return tx_sym4(p.idle4, (unsigned)(q % p.idle_len));
}

// the samples of this pull and the symbols past head they end in
static __device__ __forceinline__ unsigned tx_samples(const TxParams &p, unsigned s)
{
    return p.count[s] < p.stride ? p.count[s] : p.stride;
}

// One workgroup of 1 .. kTxPhaseMaxWaves waves per stream (the host sizes it
// by the symbols a pull can touch, so the live shape runs one wave a stream). A
// step covers blockDim.x kTxPhaseRun symbols: each thread sums its own run of
// consecutive symbols, a shuffle scan joins a wave's threads, the waves' totals
// meet in LDS, a running carry joins the steps. Wrap-around addition is
// associative, so the grouping cannot change a value.
__global__ __launch_bounds__(64 * kTxPhaseMaxWaves) void tx_phase_kernel(TxParams p)
{
    __shared__ uint32_t s_total[kTxPhaseMaxWaves];
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64, n_waves = blockDim.x / 64;
    const unsigned s = blockIdx.x;   // the grid is n_streams blocks
    const TxState t = tx_load(p, s);
    const unsigned m = tx_samples(p, s);
    // PHI(head + d) for 1 <= d <= d_end: the symbols 0 .. d_end - 1 are summed
    unsigned d_end = (t.offset + m) >> p.log2n;
    if (d_end > p.work_stride - 1) d_end = p.work_stride - 1;   // cannot happen: (n - 1 + stride) / n
    const unsigned hm = (unsigned)(t.head % p.ring_symbols), im = (unsigned)(t.head % p.idle_len);
    const uint8_t *ring = p.ring + (size_t)s * p.ring_symbols;
    uint32_t *work = p.work + (size_t)s * p.work_stride;
    if (tid == 0) work[0] = hm;
    uint32_t carry = t.phase;
    const unsigned span = blockDim.x * kTxPhaseRun;
    for (unsigned base = 0; base < d_end; base += span) {   // the same for every thread: the barriers are uniform
        const unsigned d0 = base + (unsigned)tid * kTxPhaseRun;
        uint32_t v[kTxPhaseRun], sum = 0;
#pragma unroll
        for (int j = 0; j < kTxPhaseRun; ++j) {
            const unsigned d = d0 + (unsigned)j;
            unsigned sym = 16;   // no tone: inc 0
            if (d < d_end)
                sym = t.head + d < t.tail ? ring[(hm + d) % p.ring_symbols] & 15u
                                          : tx_sym4(p.idle4, (im + d) % p.idle_len);   // hm + d, im + d < 2^32
            v[j] = p.n * tx_inc(p, sym);
            sum += v[j];
        }
        uint32_t x = sum;
        for (int k = 1; k < 64; k <<= 1) {
            const uint32_t y = __shfl_up(x, k);
            if (lane >= k) x += y;
        }
        if (lane == 63) s_total[wave] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kTxPhaseMaxWaves; ++w) {
            const uint32_t tot = w < n_waves ? s_total[w] : 0u;
            before += w < wave ? tot : 0u;
            all += tot;
        }
        __syncthreads();   // s_total is rewritten by the next step
        uint32_t run = carry + before + x - sum;   // PHI of the thread's first symbol
#pragma unroll
        for (int j = 0; j < kTxPhaseRun; ++j) {
            run += v[j];
            if (d0 + (unsigned)j < d_end) work[d0 + (unsigned)j + 1] = run;
        }
        carry += all;
    }
}

__global__ __launch_bounds__(kRowThreads) void tx_samples_kernel(TxParams p, unsigned bps)
{
    const unsigned s = blockIdx.x / bps;
    const unsigned x0 = ((blockIdx.x - s * bps) * kRowThreads + threadIdx.x) * 8u;
    const unsigned m = tx_samples(p, s);
    if (x0 >= m) return;
    const TxState t = tx_load(p, s);
    const uint8_t *ring = p.ring + (size_t)s * p.ring_symbols;
    const uint32_t *work = p.work + (size_t)s * p.work_stride;
    const unsigned hm = work[0] < p.ring_symbols ? work[0] : 0u;
    const unsigned last = x0 + 7 < m ? x0 + 7 : m - 1;
    const unsigned y0 = t.offset + x0;
    const unsigned d0 = y0 >> p.log2n, d1 = (t.offset + last) >> p.log2n;   // d1 <= d0 + 1 < work_stride
    const uint32_t inc0 = tx_inc(p, tx_symbol(p, t, ring, hm, d0));
    const uint32_t phi0 = d0 ? work[d0] : t.phase;
    uint32_t inc1 = inc0, phi1 = phi0;
    if (d1 != d0) {
        inc1 = tx_inc(p, tx_symbol(p, t, ring, hm, d1));
        phi1 = work[d1];
    }
    const uint64_t ns = mix64(p.seed + ((uint64_t)s + 1) * kSynthGamma);
    const uint64_t c0 = t.head * p.n + y0 + 1;
    int16_t out[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const unsigned y = y0 + (unsigned)r;
        const bool second = (y >> p.log2n) != d0;
        const uint32_t ph = (second ? phi1 : phi0) + (y & (p.n - 1)) * (second ? inc1 : inc0);
        const int32_t tone = (p.amplitude * (int32_t)p.lut[ph >> 18] + 16384) >> 15;
        const uint64_t d = mix64(ns + (c0 + (uint64_t)r) * kSynthGamma);
        const int64_t u = (int64_t)((d & 0xFFFF) + ((d >> 16) & 0xFFFF) + ((d >> 32) & 0xFFFF) + (d >> 48));
        const int64_t noise = ((u - 131070) * (int64_t)p.sigma * 113512) >> 32;
        int64_t v = (int64_t)tone + noise;
        v = v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
        out[r] = (int16_t)v;
    }
    int16_t *dst = p.pcm + (size_t)s * p.stride + x0;
    if (x0 + 8 <= m) {
        uint4 pk;
        pk.x = (uint16_t)out[0] | ((uint32_t)(uint16_t)out[1] << 16);
        pk.y = (uint16_t)out[2] | ((uint32_t)(uint16_t)out[3] << 16);
        pk.z = (uint16_t)out[4] | ((uint32_t)(uint16_t)out[5] << 16);
        pk.w = (uint16_t)out[6] | ((uint32_t)(uint16_t)out[7] << 16);
        *reinterpret_cast<uint4 *>(dst) = pk;
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (x0 + (unsigned)r < m) dst[r] = out[r];
    }
}

__global__ __launch_bounds__(kRowThreads) void tx_state_kernel(TxParams p)
{
    const unsigned long long s64 = (unsigned long long)blockIdx.x * kRowThreads + threadIdx.x;
    if (s64 >= p.n_streams) return;
    const unsigned s = (unsigned)s64;
    const TxState t = tx_load(p, s);
    const unsigned y_end = t.offset + tx_samples(p, s);
    unsigned d_end = y_end >> p.log2n;
    if (d_end > p.work_stride - 1) d_end = p.work_stride - 1;
    demod_tx_stream_state_t *st = p.state + s;
    const unsigned long long head = t.head + d_end;
    const unsigned offset = y_end & (p.n - 1);
    const unsigned long long least = head + (offset > 0 ? 1u : 0u);
    // a pull that ends inside an idle symbol queues it: the next pull reads it from the ring
    if (offset > 0 && head >= t.tail)
        p.ring[(size_t)s * p.ring_symbols + (size_t)(head % p.ring_symbols)] =
            (uint8_t)tx_sym4(p.idle4, (unsigned)(head % p.idle_len));
    st->head = head;
    st->tail = t.tail > least ? t.tail : least;
    st->offset = offset;
    st->phase = d_end ? p.work[(size_t)s * p.work_stride + d_end] : t.phase;
}

hipError_t launch_tx_modulate(const TxParams &p, hipStream_t s)
{
    const unsigned S = p.n_streams;
    // a wave covers 64 kTxPhaseRun symbols a step: as many waves as one step of the longest pull takes
    const unsigned per_wave = 64 * kTxPhaseRun, want = (p.work_stride - 1 + per_wave - 1) / per_wave;
    const unsigned waves = want < (unsigned)kTxPhaseMaxWaves ? (want ? want : 1u) : (unsigned)kTxPhaseMaxWaves;
    hipLaunchKernelGGL(tx_phase_kernel, dim3(S), dim3(64 * waves), 0, s, p);
    const unsigned bps = (p.stride / 8 + kRowThreads - 1) / kRowThreads;   // S bps <= 2^31 / 2048 + S
    hipLaunchKernelGGL(tx_samples_kernel, dim3(S * bps), dim3(kRowThreads), 0, s, p, bps);
    hipLaunchKernelGGL(tx_state_kernel, dim3((S + kRowThreads - 1) / kRowThreads), dim3(kRowThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace fskd
