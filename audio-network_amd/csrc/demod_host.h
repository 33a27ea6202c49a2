// demod_host.h — what the host layer's files share (private): demod_api.cpp
// (handle, batch and streaming entry points), demod_acquire.cpp (acquisition
// and the frame scans on the detector's outputs), demod_frames.cpp (the stages
// over a scan's rows), demod_streams.cpp (many streams behind one handle),
// demod_rx.cpp and demod_tx.cpp (receiver and transmitter: stages and handle).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../include/demod.h"
#include "demod_internal.h"
#include "frame_shape.h"
#include "plan.h"

// Makes `dev` current for the scope of an entry point and restores the
// caller's current device on return (the ABI must not leave the calling
// thread on another device).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) {
            (void)hipGetLastError();
            prev = -1;
        }
        if (prev != dev) err = hipSetDevice(dev);
    }
    ~DeviceGuard()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

#define HIP_TRY(x)                                                 \
    do {                                                           \
        hipError_t _e = (x);                                       \
        if (_e != hipSuccess) {                                    \
            std::fprintf(stderr, "fskdemod: %s failed: %s\n", #x,  \
                         hipGetErrorString(_e));                   \
            return DEMOD_DEVICE_ERROR;                             \
        }                                                          \
    } while (0)

namespace fskd {

// A buffer that owns its allocation: device memory, pinned host memory, or
// mapped coherent pinned memory (uncached on the device) with the device's
// view of it. The only place the host layer allocates and frees buffers.
enum class Mem { Device, Pinned, Mapped };

template <class T, Mem M>
struct Buf {
    T *p = nullptr;   // Device: the device pointer; Pinned / Mapped: the host pointer
    T *d = nullptr;   // Mapped: the device view of p
    size_t cap = 0;   // elements

    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }

    void release()
    {
        if (p) (void)(M == Mem::Device ? hipFree(p) : hipHostFree(p));
        p = d = nullptr;
        cap = 0;
    }
    // Room for `count` elements: a buffer that has it stays, else it is
    // replaced (contents dropped) by one of count + slack.
    hipError_t reserve(size_t count, size_t slack = 0)
    {
        if (count <= cap) return hipSuccess;
        release();
        const size_t bytes = (count + slack) * sizeof(T);
        hipError_t e = M == Mem::Device   ? hipMalloc(&p, bytes)
                       : M == Mem::Pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault)
                                          : hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess && M == Mem::Mapped) e = hipHostGetDevicePointer((void **)&d, p, 0);
        if (e == hipSuccess) cap = count + slack;
        return e;
    }
};
template <class T> using DevBuf = Buf<T, Mem::Device>;
template <class T> using PinnedBuf = Buf<T, Mem::Pinned>;
template <class T> using MappedBuf = Buf<T, Mem::Mapped>;

// Symbols [windows] and magnitudes [windows][k] grow together.
template <Mem M>
inline hipError_t reserve_outputs(Buf<uint8_t, M> &sym, Buf<float, M> &mag, size_t windows,
                                  size_t slack, size_t k)
{
    sym.release();
    mag.release();
    const hipError_t e = sym.reserve(windows, slack);
    return e != hipSuccess ? e : mag.reserve((windows + slack) * k);
}

// Measurement switches, read from the environment once at demod_create
// (FSKD_NO_ZERO_COPY alone at the handle's first packet-sized host call, as
// include/demod.h documents).
struct Switches {
    bool no_rescue = false;        // FSKD_NO_RESCUE=1: the decision rescue off
    bool rescue_launch = true;     // FSKD_NO_RESCUE=flags: false, flag only (the symbols keep bit 7:
                                   // counting them is how bench.py reports the rate)
    bool rescue_kernel_forced = false;  // FSKD_RESCUE_LAUNCH=1: the rescue launch everywhere
    bool rescue_seg = true;        // FSKD_RESCUE_SEG=0: false, every flagged row to the exact chain
    bool wb_bursts = true;         // FSKD_WB_BURSTS=0: false, large outputs as the round-2 launch slices
    int wb_force = 0;              // FSKD_WB_BURSTS=<n >= 1>: n bursts on every hop = n batch
    bool fft_pmask = true;         // FSKD_FFT_PMASK=0: false, the full post-pass on tones-only batches
    bool streams_mapped = false;   // FSKD_STREAMS_MAPPED=1: demod_streams stages in mapped memory
};

}  // namespace fskd

struct demod {
    demod_cfg_t cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    fskd::Plan plan;            // the tone plan (error_model.cpp build_plan)
    fskd::ErrModel em;          // the decision rescue's thresholds (zero when it is off)
    fskd::Switches sw;
    bool rescue = false;        // decision rescue (rescue.hip): K >= 2 and not switched off
    // the plan's tables on the device
    fskd::DevBuf<float4> d_rot;    // [k][g]
    fskd::DevBuf<double> d_rot64;  // in-kernel rescue, first step: [k][16][4] segment rotations in double
    fskd::DevBuf<float> d_tw512;   // FFT detector tables
    fskd::DevBuf<float> d_tw1024;
    fskd::DevBuf<int> d_bins;
    fskd::DevBuf<double> d_rtw;    // FFT: radix-2 twiddles (cos, sin)(-2 pi j / len), [n - 1]
    // launch templates: what is constant for the handle (demod_api.cpp enqueue_*)
    fskd::GoertzelParams gp;
    fskd::FftParams fp;
    fskd::RescueParams rp;
    // staging for host-pointer calls
    fskd::DevBuf<int16_t> d_in;
    fskd::DevBuf<uint8_t> d_sym;        // d_sym.cap windows: d_mag grows with it
    fskd::DevBuf<float> d_mag;
    // demod_acquire: workspace, result and symbol-rate output (first use)
    fskd::DevBuf<unsigned char> d_acq_work;
    fskd::DevBuf<demod_acquire_result_t> d_acq_res;
    fskd::DevBuf<uint8_t> d_acq_out;
    // demod_acquire_segments: the tables, workspace, results and rows (first use)
    fskd::DevBuf<uint64_t> d_seg_first;
    fskd::DevBuf<uint32_t> d_seg_count;
    fskd::DevBuf<unsigned char> d_seg_work;
    fskd::DevBuf<demod_acquire_result_t> d_seg_res;
    fskd::DevBuf<uint8_t> d_seg_out;
    fskd::PinnedBuf<uint8_t> h_seg_out; // the rows on their way to the caller's [S][cap]
    // demod_frames: workspace, result, hits and payload rows (first use)
    fskd::DevBuf<unsigned char> d_frm_work;
    fskd::DevBuf<demod_frames_result_t> d_frm_res;
    fskd::DevBuf<demod_frame_hit_t> d_frm_hits;
    fskd::DevBuf<uint8_t> d_frm_payload;
    fskd::DevBuf<uint8_t> d_frm_packed;
    // demod_frames_segments: results and rows (first use); the tables and the
    // workspace are demod_acquire_segments' (d_seg_first, d_seg_count, d_seg_work)
    fskd::DevBuf<demod_frames_result_t> d_fsg_res;
    fskd::DevBuf<demod_frame_hit_t> d_fsg_hits;
    fskd::DevBuf<uint8_t> d_fsg_payload;
    fskd::DevBuf<uint8_t> d_fsg_packed;
    fskd::PinnedBuf<demod_frame_hit_t> h_fsg_hits;   // the rows on their way to the caller's [S][max_frames]
    fskd::PinnedBuf<uint8_t> h_fsg_payload;
    fskd::PinnedBuf<uint8_t> h_fsg_packed;
    // demod_frames_checked: the check's outputs over demod_frames' rows (d_frm_*), then
    // the kept rows' hits and lengths side by side (first use)
    fskd::DevBuf<demod_frame_check_t> d_chk_check;
    fskd::DevBuf<uint32_t> d_chk_kept;
    fskd::DevBuf<uint8_t> d_chk_body;
    fskd::DevBuf<demod_frames_check_result_t> d_chk_sum;
    fskd::DevBuf<demod_frame_hit_t> d_chk_hits;
    fskd::DevBuf<uint32_t> d_chk_len;
    std::vector<uint8_t> h_chk_body;    // the body rows on their way to the caller's bytes
    // demod_frames_coded: the decoded rows, their reports and the survivor words (first use)
    fskd::DevBuf<uint8_t> d_fec_rows;
    fskd::DevBuf<demod_frame_decode_t> d_fec_decode;
    fskd::DevBuf<unsigned char> d_fec_work;
    fskd::DevBuf<demod_frame_rs_t> d_rs;
    fskd::DevBuf<uint64_t> d_erase;     // with a level: the rows' erasure masks and the decoder's second records
    fskd::DevBuf<demod_frame_erase_t> d_erec;
    fskd::PinnedBuf<int16_t> h_in;      // pinned staging for small host calls
    fskd::PinnedBuf<uint8_t> h_sym;
    fskd::PinnedBuf<float> h_mag;       // [h_sym.cap][k]
    // packet-sized calls: the kernel reads the window samples from, and
    // writes its results to, mapped coherent host memory (no copies)
    int zc = 0;                         // 0: not set up, 1: ready, -1: unavailable
    fskd::MappedBuf<int16_t> z_in;      // [kZeroCopySamples]
    fskd::MappedBuf<uint8_t> z_sym;
    fskd::MappedBuf<float> z_mag;
    hipStream_t copy_stream = nullptr;  // H2D of large host-pointer calls
    hipEvent_t copied[2] = {};          // device slot b holds its chunk
    hipEvent_t consumed[2] = {};        // the kernel reading slot b has run
    // streaming carry (mono samples not yet consumed by a complete window)
    std::vector<int16_t> carry;
    std::vector<int16_t> scratch;
    // lead-in: mono frames still to drop at the start of the stream (cfg.lead_in
    // after demod_create / demod_reset)
    size_t skip = 0;
};

namespace fskd {

constexpr size_t kSmallHostSamples = 1 << 21;  // 4 MiB: pinned-staging path

// Enqueue the detector kernel on device-resident windows.
int enqueue_batch(demod_t *st, const int16_t *d_pcm, size_t n_windows, uint8_t *d_sym, float *d_mag,
                  hipStream_t s);
// Host samples [n_samples] -> device, kernel, results -> host (synchronous).
int run_host(demod_t *st, const int16_t *pcm, size_t n_samples, size_t n_windows, uint8_t *symbols,
             float *mags);
// The pinned staging buffers of small host calls.
int ensure_host(demod_t *st, size_t samples, size_t windows);
// The device staging of host-pointer calls: st->d_in, st->d_sym and st->d_mag.
int ensure_dev(demod_t *st, size_t samples, size_t windows, bool mags);
// Device or managed memory (a host pointer, or one the runtime does not know: false).
bool is_device_ptr(const void *p);

// ---- what the entry points on the detector's outputs share (demod_acquire.cpp and on) ----

// Every pointer on an 8-byte (4-byte) boundary; a null pointer is.
template <class... T> static inline bool aligned8(const T *...p) { return (((uintptr_t)p | ...) & 7) == 0; }
template <class... T> static inline bool aligned4(const T *...p) { return (((uintptr_t)p | ...) & 3) == 0; }

// R = n / hop when it divides and is at most DEMOD_MAX_PHASES, else 0 (n and
// hop are powers of two for every valid configuration, so R is one)
static inline uint32_t acquire_phases(const demod_cfg_t &c)
{
    if (c.hop == 0 || c.n % c.hop != 0) return 0;
    const uint32_t r = c.n / c.hop;
    return (r >= 1 && r <= DEMOD_MAX_PHASES && (r & (r - 1)) == 0) ? r : 0;
}

// Bytes of a packed row: N symbols of `bits` bits, MSB first, the last byte padded
static inline size_t packed_row_bytes(size_t N, size_t bits) { return (N * bits + 7) / 8; }

// Rows a synchronous wrapper keeps on the device for `windows` windows: the
// caller's cap, or every row there can be. Acquisition writes one symbol per R
// windows (n_out <= ceil(W / R)); complete hits are starts on one phase whose
// frame fits, so W / R + 1 bounds them too.
static inline size_t hit_cap(size_t cap, size_t windows, uint32_t R) { return std::min(cap, windows / R + 1); }

// Groups (segments, streams) of max_frames rows each: 1 .. DEMOD_MAX_SEGMENTS groups and fewer than 2^31
// rows in all. The frame scans take max_frames == 0 (they only count); the stages over rows do not.
static inline bool group_rows_ok(size_t n_groups, size_t max_frames, bool rows_may_be_zero)
{
    if (n_groups == 0 || n_groups > DEMOD_MAX_SEGMENTS || max_frames > 0x7FFFFFFF) return false;
    return max_frames ? (unsigned long long)n_groups * max_frames <= 0x7FFFFFFFull : rows_may_be_zero;
}

// The configuration's R when the shape and the sync word are acceptable, else
// 0. whole: the batch is acquired as one stream and needs R windows (a segment
// with fewer is an outcome of the segmented call, not a refusal).
static inline uint32_t acquire_args(const demod_cfg_t &cfg, size_t n_windows, const uint8_t *sync,
                                    size_t sync_len, uint32_t max_errors, bool whole)
{
    const uint32_t R = acquire_phases(cfg);
    if (R == 0 || (whole && n_windows < R) || n_windows > 0x7FFFFFFF) return 0;
    if (sync_len > DEMOD_MAX_SYNC || (sync_len && (!sync || max_errors >= sync_len))) return 0;
    for (size_t i = 0; i < sync_len; ++i)
        if (sync[i] >= cfg.k) return 0;
    return R;
}

// R when a frame scan of these arguments is acceptable, else 0: what
// acquire_args refuses, no word, or a frame of 2^31 windows or more.
static inline uint32_t frames_args(const demod_cfg_t &cfg, size_t n_windows, const uint8_t *sync,
                                        size_t sync_len, uint32_t max_errors, size_t frame_symbols,
                                        size_t max_frames, bool whole)
{
    const uint32_t R = acquire_args(cfg, n_windows, sync, sync_len, max_errors, whole);
    if (R == 0 || sync_len == 0 || max_frames > 0x7FFFFFFF) return 0;
    if (frame_symbols > 0x7FFFFFFF || (sync_len + frame_symbols) * R > 0x7FFFFFFF) return 0;
    return R;
}

// The synchronous wrappers' first half, on st->stream: the batch's samples on
// the device (host samples are copied to st->d_in, a device pointer is read in
// place), then the detector into st->d_sym and st->d_mag.
static inline int stage_and_detect(demod_t *st, const int16_t *pcm, size_t n_windows)
{
    const size_t n_samples = (n_windows - 1) * st->cfg.hop + st->cfg.n;
    const bool din = is_device_ptr(pcm);
    int rc;
    if ((rc = ensure_dev(st, din ? 0 : n_samples, n_windows, true)) != DEMOD_OK) return rc;
    if (!din)
        HIP_TRY(hipMemcpyAsync(st->d_in.p, pcm, n_samples * sizeof(int16_t), hipMemcpyHostToDevice,
                               st->stream));
    rc = enqueue_batch(st, din ? pcm : st->d_in.p, n_windows, st->d_sym.p, st->d_mag.p, st->stream);
    return rc < 0 ? rc : DEMOD_OK;
}

// What every stage over a scan's rows asks of its call: the configuration's R, the groups and rows, the word's
// length and the row's shape (fec 0: the scan's packed rows). R with the shape filled, or 0 for what they refuse.
static inline uint32_t stage_shape(const demod_cfg_t &cfg, size_t n_groups, size_t max_frames, size_t sync_len,
                                   size_t frame_symbols, int len_bytes, int crc, int fec, frame_shape &s)
{
    const uint32_t R = acquire_phases(cfg);
    if (R == 0 || !group_rows_ok(n_groups, max_frames, false) || sync_len == 0 || sync_len > DEMOD_MAX_SYNC)
        return 0;
    const int bits = demod_bits_per_symbol(cfg.k);
    return frame_shape_fill(&s, bits, cfg.k == (1u << bits), frame_symbols, len_bytes, crc, fec) ? 0 : R;
}

// What the erasure masks' producer asks of its call beside the level and the pointers (include/demod.h "erasure
// decoding"): K one of 2, 4, 8, 16, the groups and rows, the word's length and plain rows of B bytes. The entries
// that run the producer for a level ask the same before they queue anything. R with B filled, or 0.
static inline uint32_t erasures_shape(const demod_cfg_t &cfg, size_t n_groups, size_t max_frames, size_t sync_len,
                                      size_t frame_symbols, unsigned &B)
{
    const uint32_t R = acquire_phases(cfg);
    if (R == 0 || !group_rows_ok(n_groups, max_frames, false) || sync_len == 0 || sync_len > DEMOD_MAX_SYNC)
        return 0;
    if (cfg.k != 2 && cfg.k != 4 && cfg.k != 8 && cfg.k != 16) return 0;
    B = frame_plain_row_bytes(demod_bits_per_symbol(cfg.k), frame_symbols);
    if (B == 0 || (sync_len + frame_symbols) * (size_t)R > 0x7FFFFFFF) return 0;
    return R;
}

// The shape fields FramesCheckParams, FramesFecParams and RxCollectParams name alike, from the row's shape
// (frame_shape.h) and the call's rows, R and L. What a block calls its own (its groups, row_bytes, steps,
// fec_depth) its entry point sets; FramesRsParams, with no span on the air, is filled there whole.
template <class P>
static inline void fill_shape_fields(P &p, const frame_shape &s, size_t max_frames, uint32_t R, size_t sync_len)
{
    p.max_frames = (unsigned)max_frames;
    p.max_len = s.max_len;
    p.len_bytes = s.len_bytes;
    p.crc_bytes = s.crc_bytes;
    p.bits = s.bits;
    p.phases = (int)R;
    p.sync_len = (int)sync_len;
    p.fec = s.fec;
    p.parity = s.parity;
}

// poly, init and xpow8[] of the CRC of crc_bytes bytes (FramesCheckParams, TxParams): the register in the top
// 8 c bits of the word; x^8, then its squares mod P (Horner over the square's own coefficients, highest first).
template <class P>
static inline void fill_crc_fields(P &p, int crc_bytes)
{
    static_assert(DEMOD_MAX_FRAME_PAYLOAD + 2 < (1 << kCrcPowBits), "bytes after a lane's chunk");
    p.poly = crc_bytes == 2 ? 0x1021u << 16 : 0x04C11DB7u;
    p.init = crc_bytes == 2 ? 0xFFFFu << 16 : 0xFFFFFFFFu;
    const int width = 8 * crc_bytes;
    p.xpow8[0] = 1u << (32 - width + 8);
    for (int j = 1; j < kCrcPowBits; ++j) {
        const uint32_t a = p.xpow8[j - 1];
        uint32_t r = 0, b = a;
        for (int i = 0; i < width; ++i, b <<= 1)
            r = (r << 1) ^ ((r >> 31) ? p.poly : 0u) ^ ((b >> 31) ? a : 0u);
        p.xpow8[j] = r;
    }
}

// demod_streams.cpp: the staging half of a push, shared by demod_streams_push
// and demod_rx_push (demod_rx.cpp). After streams_check (plan.h) has admitted
// the packets and laid the batch out: streams_stage, the batch, then
// streams_commit, or streams_unstage when the batch failed.
struct StreamsStage {
    size_t W = 0;                 // the windows the streams emit
    size_t Wb = 0;                // the batch's windows, the straddling ones included
    size_t samples = 0;           // staged samples, (Wb - 1) hop + n; 0 without a window
    int16_t *base = nullptr;      // the staging buffer (host view); stream s's run at first[s] hop
    const size_t *first = nullptr;  // [S] batch window of each stream's first
};
int streams_stage(demod_streams_t *ms, const int16_t *const *pcm, const size_t *n_frames, size_t W,
                  size_t Wb, size_t tail, StreamsStage *out);
void streams_unstage(demod_streams_t *ms, const size_t *n_frames, const StreamsStage &sg);
void streams_commit(demod_streams_t *ms, const int16_t *const *pcm, const size_t *n_frames,
                    uint32_t *counts);
demod_t *streams_detector(demod_streams_t *ms);
// The handle's layout table [S]: what streams_check fills and streams_stage reads.
size_t *streams_first(demod_streams_t *ms);
// Stage in pinned memory whatever FSKD_STREAMS_MAPPED says (the receiver copies its runs in).
void streams_copy_staging(demod_streams_t *ms);

}  // namespace fskd
