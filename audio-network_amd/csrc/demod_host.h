// demod_host.h — what the host layer's files share (private): demod_api.cpp
// (handle, batch and streaming entry points), demod_acquire.cpp (acquisition
// and frame entry points on the detector's outputs), demod_streams.cpp (many
// streams behind one handle) and demod_rx.cpp (the receiver handle).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../include/demod.h"
#include "demod_internal.h"
#include "fec_map.h"
#include "rs_ops.h"
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
