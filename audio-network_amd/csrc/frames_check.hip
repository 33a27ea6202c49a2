// frames_check.hip — checked frames (include/demod.h "checked frames",
// DESIGN.md §4.9 "Checked frames"): a pass over the rows a frame scan wrote
// (acquire_frames.hip, acquire_frames_segments.hip) that reads each row's length
// header, checks its CRC, marks rows that start inside an earlier valid frame
// and compacts the surviving rows and their data bytes. Group g owns rows
// g max_frames + i, i < nw_g = min(res[g].n_written, max_frames): the count is
// device memory, read and clamped by every launch, and every index below is
// bounded by the clamped count, max_len and the row width alone. Three
// launches whatever the counts are (two without d_body), no workspace:
//
//  check   one wave per row: wave c of a group's wpg waves takes rows c,
//          c + wpg, .. below nw_g (wave-uniform; a group without rows costs its
//          waves one load). The CRC register is kept in the top `width` bits of
//          a 32-bit word, so CRC-16 and CRC-32 share every line. Lane l runs
//          the byte-table CRC (256 entries, built in LDS by the workgroup) over
//          its contiguous chunk of ceil((h + len) / 64) bytes, lane 0 from init
//          and the others from 0; by linearity
//              crc(init, A || B) = crc(init, A) x^(8 |B|) + crc(0, B)  mod P
//          each lane multiplies its register by x^(8 bytes after its chunk)
//          (lane-local GF(2) multiply; square-and-multiply with the squares
//          x^(8 2^j) computed once on the host and passed in the parameter
//          block) and the wave XORs the 64 registers by shuffle. length, crc,
//          status.
//  select  one workgroup per group walks its rows in chunks of kAcqThreads,
//          carrying (rows OK, rows kept, max end so far) in registers. covered
//          is the exclusive prefix maximum of end over the OK rows against the
//          row's own window: a wave scan by shuffle, wave totals through LDS. A
//          kept row's rank is the rows kept before the chunk, in the waves
//          before (LDS) and in the lanes before (ballot), as frames_emit_kernel:
//          ascending by construction. covered, kept, summary. A frame's span on
//          the air is its bytes' symbols, or with fec_depth (the coded check
//          over frames_fec.hip's rows) its 2 T(len) coded bits' symbols.
//  body    one thread per data byte of the kept rows, coalesced along the byte
//          index; reads n_kept, kept and length as select and check left them.
//
// The prefix maximum is deliberately not the serial greedy hold-off: it drops a
// superset of what greedy drops, and the two differ only when frames that pass
// their CRC overlap each other. No atomics; every output byte is a function of
// the inputs alone.
#include "acquire_scan.h"
#include "crc_ops.h"

namespace fskd {

constexpr int kChkLanes = 64;
constexpr int kChkWaves = kAcqThreads / kChkLanes;
constexpr unsigned kChkMaxWaves = 16384;   // check and body: waves per call (or one per group)

static_assert(kAcqThreads == 256, "one thread builds one entry of the byte table");

static __device__ __forceinline__ unsigned group_rows(const FramesCheckParams &p, unsigned g)
{
    const unsigned long long n = p.res[g].n_written;
    return n < p.max_frames ? (unsigned)n : p.max_frames;
}

template <int WIDTH>
__global__ __launch_bounds__(kAcqThreads) void frames_check_kernel(FramesCheckParams p, unsigned wpg)
{
    __shared__ unsigned s_tab[256];
    const int t = threadIdx.x, wave = t / kChkLanes, lane = t % kChkLanes;
    {
        unsigned r = (unsigned)t << 24;
        for (int b = 0; b < 8; ++b) r = crc_xtime(r, p.poly);
        s_tab[t] = r;
    }
    __syncthreads();
    const unsigned long long gw = (unsigned long long)blockIdx.x * kChkWaves + wave;
    const unsigned long long g64 = gw / wpg;
    if (g64 >= p.n_groups) return;
    const unsigned g = (unsigned)g64, c = (unsigned)(gw % wpg);
    const unsigned nw = group_rows(p, g);
    const int h = p.len_bytes;
    for (unsigned i = c; i < nw; i += wpg) {   // the same for every lane of the wave
        const size_t r = (size_t)g * p.max_frames + i;
        const uint8_t *row = p.packed + r * p.row_bytes;
        unsigned len = row[0];
        if (h == 2) len = (len << 8) | row[1];
        len = (unsigned)__builtin_amdgcn_readfirstlane((int)len);
        unsigned crc = 0, status = DEMOD_CHECK_BAD_LENGTH;
        if (len <= p.max_len) {
            const unsigned n = (unsigned)h + len;               // <= row_bytes - crc_bytes
            const unsigned reg = crc_wave<WIDTH>(row, n, lane, p.init, p.poly, p.xpow8, s_tab);
            crc = reg >> (32 - WIDTH);
            unsigned stored = 0;
            for (int b = 0; b < p.crc_bytes; ++b) stored = (stored << 8) | row[n + b];
            status = stored == crc ? DEMOD_CHECK_OK : DEMOD_CHECK_BAD_CRC;
        }
        if (lane == 0) {
            demod_frame_check_t *out = p.check + r;
            out->length = len;
            out->crc = crc;
            out->status = status;
        }
    }
}

__global__ __launch_bounds__(kAcqThreads) void frames_select_kernel(FramesCheckParams p)
{
    __shared__ unsigned long long s_wmax[kChkWaves];
    __shared__ unsigned s_wkept[kChkWaves], s_wok[kChkWaves];
    const int t = threadIdx.x, wave = t / kChkLanes, lane = t % kChkLanes;
    const unsigned long long R = (unsigned long long)p.phases, L = (unsigned long long)p.sync_len;
    const unsigned bits = (unsigned)p.bits;
    for (unsigned g = blockIdx.x; g < p.n_groups; g += gridDim.x) {
        // the same for every thread of the block: the barriers below are uniform
        const unsigned nw = group_rows(p, g);
        const size_t row0 = (size_t)g * p.max_frames;
        unsigned n_ok = 0, n_kept = 0;
        unsigned long long carry = 0;   // max end over the OK rows of the chunks before
        for (unsigned base = 0; base < nw; base += kAcqThreads) {
            const unsigned i = base + t;
            const bool in = i < nw;
            bool ok = false;
            unsigned long long window = 0, end = 0;
            if (in && p.check[row0 + i].status == DEMOD_CHECK_OK) {
                ok = true;
                window = p.hits[row0 + i].window;
                // the frame's symbols on the air: its bytes, or coded 2 T(len) bits
                const unsigned S = checked_frame_span(p.check[row0 + i].length, (unsigned)p.len_bytes,
                                                      (unsigned)p.crc_bytes, bits, (unsigned)p.fec_depth, (unsigned)p.fec,
                                                      (unsigned)p.parity);
                end = window + (L + S) * R;
            }
            // inclusive maximum over the lanes up to this one, then over the waves before
            unsigned long long x = end;
            for (int d = 1; d < kChkLanes; d <<= 1) {
                const unsigned long long y = __shfl_up(x, d);
                if (lane >= d && y > x) x = y;
            }
            unsigned long long before = __shfl_up(x, 1);
            if (lane == 0) before = 0;
            if (lane == kChkLanes - 1) s_wmax[wave] = x;
            __syncthreads();
            unsigned long long all = carry;
            if (carry > before) before = carry;
#pragma unroll
            for (int v = 0; v < kChkWaves; ++v) {
                const unsigned long long m = s_wmax[v];
                if (v < wave && m > before) before = m;
                if (m > all) all = m;
            }
            const bool covered = ok && before > window;
            const bool keep = ok && !covered;
            const unsigned long long kb = __ballot(keep), ob = __ballot(ok);
            if (lane == 0) {
                s_wkept[wave] = (unsigned)__popcll(kb);
                s_wok[wave] = (unsigned)__popcll(ob);
            }
            __syncthreads();
            unsigned k_before = 0, k_all = 0, ok_all = 0;
#pragma unroll
            for (int v = 0; v < kChkWaves; ++v) {
                const unsigned n = s_wkept[v];
                k_before += v < wave ? n : 0;
                k_all += n;
                ok_all += s_wok[v];
            }
            if (in) p.check[row0 + i].covered = covered ? 1u : 0u;
            if (keep)
                p.kept[row0 + n_kept + k_before + (unsigned)__popcll(kb & ((1ull << lane) - 1ull))] = i;
            n_kept += k_all;
            n_ok += ok_all;
            carry = all;
        }
        if (t == 0) {
            demod_frames_check_result_t s;
            s.n_checked = nw;
            s.n_valid = n_ok;
            s.n_kept = n_kept;
            s.reserved = 0;
            p.summary[g] = s;
        }
    }
}

// wpg waves per group: wave c of group g takes bytes 64 c + lane, + 64 wpg, ..
__global__ __launch_bounds__(kAcqThreads) void frames_body_kernel(FramesCheckParams p, unsigned wpg)
{
    const int wave = threadIdx.x / kChkLanes, lane = threadIdx.x % kChkLanes;
    const unsigned long long gw = (unsigned long long)blockIdx.x * kChkWaves + wave;
    const unsigned long long g = gw / wpg, c = gw % wpg;
    if (g >= p.n_groups) return;
    unsigned long long nk = p.summary[g].n_kept;   // select's, of this call
    if (nk > p.max_frames) nk = p.max_frames;
    const unsigned long long M = p.max_len, B = p.row_bytes;
    const size_t row0 = (size_t)g * p.max_frames;
    const unsigned long long step = (unsigned long long)wpg * kChkLanes;
    for (unsigned long long e = c * kChkLanes + lane; e < nk * M; e += step) {
        const unsigned long long r = e / M, b = e - r * M;
        const unsigned i = p.kept[row0 + r];
        if (i < p.max_frames && b < p.check[row0 + i].length)
            p.body[(row0 + r) * M + b] = p.packed[(row0 + i) * B + p.len_bytes + b];
    }
}

hipError_t launch_frames_check(const FramesCheckParams &p, hipStream_t s)
{
    const unsigned S = p.n_groups;
    const unsigned most = kChkMaxWaves / S ? kChkMaxWaves / S : 1;
    {
        const unsigned wpg = p.max_frames < most ? p.max_frames : most;
        const unsigned long long blocks = ((unsigned long long)S * wpg + kChkWaves - 1) / kChkWaves;
        if (p.crc_bytes == 2)
            hipLaunchKernelGGL(frames_check_kernel<16>, dim3((unsigned)blocks), dim3(kAcqThreads), 0, s, p, wpg);
        else
            hipLaunchKernelGGL(frames_check_kernel<32>, dim3((unsigned)blocks), dim3(kAcqThreads), 0, s, p, wpg);
    }
    hipLaunchKernelGGL(frames_select_kernel, dim3(S), dim3(kAcqThreads), 0, s, p);
    if (p.body && p.max_len > 0) {
        const unsigned long long want =
            ((unsigned long long)p.max_frames * p.max_len + kChkLanes - 1) / kChkLanes;
        const unsigned wpg = (unsigned)(want < most ? want : most);
        const unsigned long long blocks = ((unsigned long long)S * wpg + kChkWaves - 1) / kChkWaves;
        hipLaunchKernelGGL(frames_body_kernel, dim3((unsigned)blocks), dim3(kAcqThreads), 0, s, p, wpg);
    }
    return hipGetLastError();
}

__global__ __launch_bounds__(kAcqThreads) void frames_kept_rows_kernel(
    const demod_frame_hit_t *hits, const demod_frame_check_t *check, const uint32_t *kept,
    const demod_frames_check_result_t *summary, unsigned max_frames, demod_frame_hit_t *out_hits,
    uint32_t *out_len)
{
    unsigned long long nk = summary->n_kept;
    if (nk > max_frames) nk = max_frames;
    const unsigned long long step = (unsigned long long)gridDim.x * kAcqThreads;
    for (unsigned long long r = (unsigned long long)blockIdx.x * kAcqThreads + threadIdx.x; r < nk; r += step) {
        const unsigned i = kept[r];
        if (i >= max_frames) continue;
        out_hits[r] = hits[i];
        out_len[r] = check[i].length;
    }
}

hipError_t launch_frames_kept_rows(const demod_frame_hit_t *hits, const demod_frame_check_t *check,
                                   const uint32_t *kept, const demod_frames_check_result_t *summary,
                                   unsigned max_frames, demod_frame_hit_t *out_hits, uint32_t *out_len,
                                   hipStream_t s)
{
    const unsigned blocks = (max_frames + kAcqThreads - 1) / kAcqThreads;
    hipLaunchKernelGGL(frames_kept_rows_kernel, dim3(blocks < 1024 ? blocks : 1024), dim3(kAcqThreads), 0, s,
                       hits, check, kept, summary, max_frames, out_hits, out_len);
    return hipGetLastError();
}

}  // namespace fskd
