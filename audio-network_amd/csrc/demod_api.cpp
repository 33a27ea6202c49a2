// demod_api.cpp — C ABI host layer of libfskdemod.so (include/demod.h): the
// handle, the batch and streaming entry points, the segment layout, synth,
// framing, strerror and version. What runs on the detector's outputs is
// demod_acquire.cpp (acquisition, frame scans) and demod_frames.cpp (the stages
// over a scan's rows); many streams, demod_streams.cpp.
//
// Handle lifecycle mirrors the Opus decoder the reference receiver drives
// (opus_decoder_create/destroy, hardware/src/playback.cpp:67-74); streaming
// intake mirrors the per-packet call at playback.cpp:115-122, where
// demodulate(pcm, nSamplesDecoded) would consume opus_decode's output.
// Errors are returned (no abort(), unlike OPUS_ERROR_CHECK playback.cpp:16-22).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "demod_host.h"
#include "stream_stage.h"

using namespace fskd;

// The measurement switches of the environment (Switches, demod_host.h).
static Switches read_switches()
{
    const auto is = [](const char *v, const char *s) { return v && std::strcmp(v, s) == 0; };
    Switches sw;
    const char *no_rescue = std::getenv("FSKD_NO_RESCUE");
    sw.no_rescue = no_rescue && no_rescue[0] == '1';
    sw.rescue_launch = !is(no_rescue, "flags");
    sw.rescue_kernel_forced = is(std::getenv("FSKD_RESCUE_LAUNCH"), "1");
    sw.rescue_seg = !is(std::getenv("FSKD_RESCUE_SEG"), "0");
    const char *wb = std::getenv("FSKD_WB_BURSTS");
    sw.wb_bursts = !is(wb, "0");
    if (wb && std::atoi(wb) > 0) sw.wb_force = std::min(std::atoi(wb), 64);
    sw.fft_pmask = !is(std::getenv("FSKD_FFT_PMASK"), "0");
    const char *mp = std::getenv("FSKD_STREAMS_MAPPED");
    sw.streams_mapped = mp && mp[0] == '1';
    return sw;
}

// A host table on the device (an empty one stays off it).
template <class T>
static hipError_t upload(DevBuf<T> &b, const std::vector<T> &v)
{
    if (v.empty()) return hipSuccess;
    const hipError_t e = b.reserve(v.size());
    return e != hipSuccess ? e : hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// The direct Goertzel-family kernels at n = 1024 (plain bank, fold, residue;
// any hop without segment sharing) re-decide their flagged windows inside the
// detector kernel (rescue_rows, rescue_rows.h) from the tile they hold in
// LDS: no rescue launch. Segment-shared windows (SLIDE, fold_slide_kernel)
// and other window lengths keep rescue_kernel's launch; the FFT detector
// always rescues in its own kernel (rescue_fft.h).
static bool rescue_in_kernel(const demod_t *st)
{
    const Plan &pl = st->plan;
    // the residue detector's plans take the rescue launch (round 5): its first
    // pass by the residue fold lives there (its per-lane class data would not
    // fit the residue kernels' registers). Worst case (every window a near
    // tie) 2.09 -> 1.59 ms per 2^20 8-FSK windows on bins 32 + 9i; the extra
    // launch costs the clean step 0.4-0.75 % (0.3446 vs 0.3420 ms,
    // profiles/round5/r5zg/, r5zh/)
    if (pl.detector == kDetResidue && pl.fold64 == 2) return false;
    return pl.detector != kDetFft && pl.log2g == 4 && st->gp.slide_wt == 0 && !st->sw.rescue_kernel_forced;
}

// The launch templates: everything a launch's parameters hold that is
// constant for the handle. Zeroed first, so the kernarg's padding bytes are
// defined; enqueue_* copy one and set the per-call fields.
static void build_launch_templates(demod_t *st)
{
    const demod_cfg_t &c = st->cfg;
    const Plan &pl = st->plan;
    const ErrModel &m = st->em;
    const bool rescue_on = st->rescue && st->sw.rescue_launch;

    GoertzelParams &g = st->gp;
    std::memset(&g, 0, sizeof(g));
    g.hop = c.hop;
    g.log2g = pl.log2g;
    g.k = (int)c.k;
    g.rot = st->d_rot.p;
    // the tone plan's fp32 constants (error_model.cpp build_plan)
    for (uint32_t k = 0; k < c.k; ++k) {
        g.coef[k] = pl.coef[k];
        g.sgn[k] = pl.sgn[k];
        g.zcls[k] = pl.zcls[k];
        g.rcoef[k] = pl.rcoef[k];
    }
    g.reinsch = pl.reinsch ? 1 : 0;
    g.dcls = pl.dcls;
    g.f16 = pl.f16 ? 1 : 0;
    g.perm = pl.perm;
    // segment-shared windows (Plan::slide): windows per tile
    const int H = (int)(c.hop / 64);
    if (pl.slide && pl.detector == kDetGoertzel)
        g.slide_wt = (64 - 16) / H + 1;  // the last window's 16 segments end in the tile
    if (pl.slide && pl.detector == kDetFolded)
        // 4 R windows (R per 16-lane group) whose 16 + (4R - 1) H segments fit the tile
        g.slide_wt = 4 * std::max(1, ((kFoldSlideSegs - 16) / H + 1) / 4);
    // overlapping windows: neighbouring tiles share lines, keep them in L2
    g.cached = c.hop < c.n ? 1 : 0;
    // adjacent tiles on one XCD: their symbol / magnitude stores fill whole
    // lines in that XCD's L2 instead of eight L2s writing back pieces of the
    // same line (2-FSK: 0.325 -> 0.305 ms), and overlapping
    // windows find their shared lines there
    g.xcd_swizzle = 1;
    g.amb_tq = (float)m.tq;
    g.amb_floor = (float)m.fl;
    g.amb_t2e = (float)m.t2e;
    g.amb_d = (float)m.amb_d;
    g.rescue_inline = rescue_on && rescue_in_kernel(st) ? 1 : 0;  // (reads g.slide_wt)
    // the in-kernel rescue's tables; its first pass's threshold^2 = t2e64 E
    // P_max, E = sum x^2 (fp32 in the kernel; error_model's safety factor
    // covers its rounding), 0: the exact chain only
    g.rot64 = st->d_rot64.p;
    g.t2e64 = m.t2e64;
    g.fold64 = pl.fold64 == 1 ? 1 : 0;  // rescue_rows: by the fold (the residue fold: the launch)

    FftParams &f = st->fp;
    std::memset(&f, 0, sizeof(f));
    f.hop = c.hop;
    f.k = (int)c.k;
    f.xcd_swizzle = 1;  // neighbouring groups on one L2: shared input lines, whole output lines
    f.tw512 = st->d_tw512.p;
    f.tw1024 = st->d_tw1024.p;
    f.bins = st->d_bins.p;
    for (uint32_t k = 0; k < c.k; ++k) f.slot[k] = pl.fft_slot[k];
    // tones only: the post-pass pair blocks holding a tone
    f.pmask = pl.detector == kDetFft && st->sw.fft_pmask ? fft_quad_pmask(pl.fft_bins, (int)c.k) : 0xFFu;
    f.amb_tq = g.amb_tq;
    f.amb_floor = g.amb_floor;
    f.amb_t2e = g.amb_t2e;
    // the FFT detector re-decides its flagged windows itself (rescue_fft.h):
    // one launch, no symbol scan
    f.rescue = rescue_on ? 1 : 0;
    f.rtw = st->d_rtw.p;
    // the rescue's first pass (tones only; with the spectrum stored every
    // flagged window takes the double FFT, whose spectrum row is the oracle's)
    f.rot64 = st->d_rot64.p;
    f.t2e64 = m.t2e64;
    f.fold64 = g.fold64;

    RescueParams &r = st->rp;
    std::memset(&r, 0, sizeof(r));
    r.hop = c.hop;
    r.n = (int)c.n;
    r.k = (int)c.k;
    for (uint32_t k = 0; k < c.k; ++k) r.coef[k] = pl.rcoef[k];
    // n = 1024: the segment-shared windows' rescue takes the first pass too
    // (the in-kernel rescue's tables and threshold, error_model.cpp)
    r.rot64 = st->d_rot64.p;
    r.t2e64 = st->d_rot64.p ? m.t2e64 : 0.0;
    r.fold64 = pl.fold64;
}

// Plan, model, upload (and the launch templates over the uploaded tables).
static int init_device_state(demod_t *st)
{
    const demod_cfg_t &c = st->cfg;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return DEMOD_NO_DEVICE;
    }
    if (c.device < 0 || c.device >= ndev) return DEMOD_NO_DEVICE;
    if (c.device >= kMaxDevices) return DEMOD_BAD_ARG;
    HIP_TRY(hipSetDevice(c.device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c.device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::fprintf(stderr, "fskdemod: device %d is %s, need gfx950 (MI355X)\n",
                     c.device, prop.gcnArchName);
        return DEMOD_NO_DEVICE;
    }
    st->device = c.device;
    HIP_TRY(hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking));
    st->sw = read_switches();

    Plan &pl = st->plan;
    build_plan(c, pl);
    st->rescue = c.k >= 2 && !st->sw.no_rescue;
    if (st->rescue) {
        // Decision rescue thresholds, derived from the plan's
        // constants and the kernels' operation sequences (error_model.cpp):
        // stage 2 flags (P_1 - P_2)^2 < t2e E_eff P_1, stage 1 the same with
        // the int16 maximum of E_eff (tq, fl); pass 0 (the in-kernel rescue's
        // first pass, n = 1024, its tables in the plan) decides a flagged row
        // where its own margin clears t2e64 E P_max.
        const bool first_pass = !pl.rot64.empty() && st->sw.rescue_seg;
        error_model(c, pl, first_pass, st->em);
    }

    if (pl.detector == kDetFft) {
        FftTables t;
        build_fft_tables(c.n, t);
        HIP_TRY(upload(st->d_rtw, t.rtw));
        HIP_TRY(upload(st->d_tw512, t.tw512));
        HIP_TRY(upload(st->d_tw1024, t.tw1024));
        HIP_TRY(upload(st->d_bins, std::vector<int>(pl.fft_bins, pl.fft_bins + c.k)));
    }
    HIP_TRY(upload(st->d_rot, pl.rot));
    HIP_TRY(upload(st->d_rot64, pl.rot64));
    build_launch_templates(st);
    return DEMOD_OK;
}

// What has an order: the handle's device is current (the callers' guard),
// both streams are idle before any buffer is released (by the handle's
// destructor, after this), events go before copy_stream, that before stream.
static void free_state(demod_t *st)
{
    if (st->stream) (void)hipStreamSynchronize(st->stream);
    if (st->copy_stream) (void)hipStreamSynchronize(st->copy_stream);
    for (int b = 0; b < 2; ++b) {
        if (st->copied[b]) (void)hipEventDestroy(st->copied[b]);
        if (st->consumed[b]) (void)hipEventDestroy(st->consumed[b]);
    }
    if (st->copy_stream) (void)hipStreamDestroy(st->copy_stream);
    if (st->stream) (void)hipStreamDestroy(st->stream);
}

extern "C" {

void demod_cfg_default(demod_cfg_t *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->fs = 48000.0;
    cfg->n = 1024;
    cfg->hop = 1024;
    cfg->k = 2;
    cfg->channels = 1;
    cfg->channel_mode = DEMOD_CH_LEFT;
    cfg->device = 0;
    cfg->method = DEMOD_METHOD_AUTO;
    cfg->freqs[0] = 1500.0;
    cfg->freqs[1] = 3000.0;
}

demod_t *demod_create(const demod_cfg_t *cfg, int *error)
{
    int rc = validate_cfg(cfg);
    demod_t *st = rc == DEMOD_OK ? new (std::nothrow) demod() : nullptr;
    if (rc == DEMOD_OK && !st) rc = DEMOD_ALLOC_FAIL;
    if (st) {
        st->cfg = *cfg;
        st->carry.reserve(cfg->n);
        st->skip = cfg->lead_in;
        DeviceGuard guard(cfg->device >= 0 ? cfg->device : 0);
        rc = init_device_state(st);
        if (rc != DEMOD_OK) {
            free_state(st);
            delete st;
            st = nullptr;
        }
    }
    if (error) *error = rc;
    return st;
}

void demod_destroy(demod_t *st)
{
    if (!st) return;
    DeviceGuard guard(st->device);
    free_state(st);
    delete st;
}

int demod_reset(demod_t *st)
{
    if (!st) return DEMOD_BAD_ARG;
    st->carry.clear();
    st->skip = st->cfg.lead_in;
    return DEMOD_OK;
}

int demod_method(const demod_t *st)
{
    if (!st) return DEMOD_BAD_ARG;
    return st->plan.detector == kDetFolded  ? DEMOD_METHOD_FOLDED
         : st->plan.detector == kDetFft     ? DEMOD_METHOD_FFT
         : st->plan.detector == kDetResidue ? DEMOD_METHOD_RESIDUE
                                            : DEMOD_METHOD_GOERTZEL;
}

int demod_slide_windows(const demod_t *st)
{
    if (!st) return DEMOD_BAD_ARG;
    return st->gp.slide_wt;
}

int demod_pending(const demod_t *st)
{
    if (!st) return DEMOD_BAD_ARG;
    return (int)st->carry.size();
}

constexpr size_t kOutChunkBytes = 10u << 20;  // symbol + magnitude bytes per detector launch
constexpr size_t kBurstBytes = 5u << 20;      // output bytes per L2 write-back burst
constexpr size_t kBurstMinBytes = 4u << 20;   // smaller outputs: no bursts

// Windows per launch of a Goertzel-family batch (enqueue_batch): outputs
// beyond ~1 MiB per XCD L2 are written back to HBM while the input still
// streams in, and the read / write turnarounds cost ~1.3 us per MiB (8-FSK:
// 336.6 us with magnitudes vs 295.3 without); up to that size they stay dirty
// in L2 and go out in one burst at the kernel's end (2-FSK's 9 MiB: +1 us).
// So batches whose outputs exceed kOutChunkBytes run as equal slices of
// 64-window multiples (8-FSK: 4 launches, 322-325 us;
// scripts/split_launch_probe.py). Overlapping windows
// (hop < n) are bound by the recurrences and L2, not by HBM turnarounds, and
// only pay the extra launches there (2-FSK hop 128: 0.466 -> 0.494 ms), so
// they stay one launch, as does the VALU-bound FFT detector.
// Round 3: such a batch runs as ONE launch that writes each XCD's L2 back in
// bursts of ~kBurstBytes of output (wb_burst, kernel_ops.h): no drain and
// ramp per slice (8-FSK 315-316 us against 331 us for the 4 slices and 337 us
// for one plain launch on one box, 309-310 / 324 / 316 us on another;
// scripts/mag_probe.hip wb). Batches from kBurstMinBytes up
// also take at least 4 bursts (2-FSK's 9 MiB: 0.3006 ms against 0.3058 ms
// with one write-back at the kernel's end, scripts/gpu_r3_wb2.sh).
// FSKD_WB_BURSTS=0 keeps the round-2 behaviour (slices, no bursts).
static size_t out_bytes(const demod_t *st, size_t n_windows, bool mags)
{
    return n_windows * (1 + (mags ? 4 * (size_t)st->cfg.k : 0));
}
static bool large_output(const demod_t *st, size_t n_windows, bool mags)
{
    return st->plan.detector != kDetFft && st->cfg.hop >= st->cfg.n && n_windows &&
           out_bytes(st, n_windows, mags) > kOutChunkBytes;
}
static size_t launch_slice(const demod_t *st, size_t n_windows, bool mags)
{
    if (!large_output(st, n_windows, mags) || st->sw.wb_bursts) return n_windows;
    const size_t parts = std::min<size_t>((out_bytes(st, n_windows, mags) + kOutChunkBytes - 1) / kOutChunkBytes, 16);
    const size_t per = (n_windows + parts - 1) / parts;
    return (per + 63) / 64 * 64;
}
static int burst_count(const demod_t *st, size_t n_windows, bool mags)
{
    const bool eligible = st->plan.detector != kDetFft && st->cfg.hop >= st->cfg.n;
    if (st->sw.wb_force && eligible) return st->sw.wb_force;
    if (!st->sw.wb_bursts || !eligible) return 0;
    const size_t out = out_bytes(st, n_windows, mags);
    if (out < kBurstMinBytes) return 0;
    return (int)std::min<size_t>(std::max<size_t>((out + kBurstBytes - 1) / kBurstBytes, 4), 64);
}

double demod_rescue_tau(const demod_t *st)
{
    if (!st || !st->rescue) return 0.0;
    return st->em.tau;
}

double demod_rescue_tau64(const demod_t *st)
{
    // every rescue at n = 1024 runs the first pass (round 5: the rescue launch
    // of segment-shared windows too, rescue.hip rescue_seg_kernel)
    if (!st || !st->rescue || !st->d_rot64.p) return 0.0;
    return st->em.tau64;
}

int demod_batch_launches(const demod_t *st, size_t n_windows, int with_mags)
{
    if (!st) return DEMOD_BAD_ARG;
    if (n_windows == 0) return 0;
    const size_t per = launch_slice(st, n_windows, with_mags != 0);
    // + the decision rescue's launch (the FFT detector rescues in the kernel)
    const size_t n = (n_windows + per - 1) / per +
                     (st->rescue && st->sw.rescue_launch && st->plan.detector != kDetFft &&
                              !rescue_in_kernel(st) ? 1 : 0);
    return n > 0x7FFFFFFF ? 0x7FFFFFFF : (int)n;
}

int demod_max_symbols(const demod_t *st, size_t n_frames)
{
    if (!st) return DEMOD_BAD_ARG;
    const size_t fresh = n_frames > st->skip ? n_frames - st->skip : 0;
    size_t w = windows_for(st->carry.size() + fresh, st->cfg.n, st->cfg.hop);
    return w > 0x7FFFFFFF ? 0x7FFFFFFF : (int)w;
}

}  // extern "C"

// The decision rescue over a batch's windows (rescue.hip), after its detector
// launches on the same stream.
static int enqueue_rescue(demod_t *st, const int16_t *d_pcm, size_t n_windows, uint8_t *d_sym,
                          float *d_mag, hipStream_t s)
{
    if (!st->rescue || !st->sw.rescue_launch || n_windows == 0 || rescue_in_kernel(st)) return DEMOD_OK;
    RescueParams r = st->rp;
    r.pcm = d_pcm;
    r.n_windows = (long long)n_windows;
    r.sym = d_sym;
    r.sym_aligned4 = ((uintptr_t)d_sym & 3) == 0;
    r.mag = d_mag;
    HIP_TRY(launch_rescue(r, s));
    return DEMOD_OK;
}

static int enqueue_fft(demod_t *st, const int16_t *d_pcm, size_t n_windows, uint8_t *d_sym,
                       float *d_mag, float *d_spec, hipStream_t s)
{
    FftParams p = st->fp;
    p.pcm = d_pcm;
    p.n_windows = (long long)n_windows;
    p.sym = d_sym;
    p.mag = d_mag;
    p.spec = d_spec;
    HIP_TRY(launch_fft_quad(p, s));
    return (int)n_windows;
}

int fskd::enqueue_batch(demod_t *st, const int16_t *d_pcm, size_t n_windows, uint8_t *d_sym,
                        float *d_mag, hipStream_t s)
{
    if (n_windows == 0) return 0;
    if (st->plan.detector == kDetFft) return enqueue_fft(st, d_pcm, n_windows, d_sym, d_mag, nullptr, s);
    GoertzelParams p = st->gp;
    const size_t per = launch_slice(st, n_windows, d_mag != nullptr);
    p.wb_bursts = burst_count(st, n_windows, d_mag != nullptr);
    for (size_t w0 = 0; w0 < n_windows; w0 += per) {
        const size_t cnt = std::min(per, n_windows - w0);
        p.pcm = d_pcm + w0 * st->cfg.hop;
        p.n_windows = (long long)cnt;
        p.sym = d_sym + w0;
        p.mag = d_mag ? d_mag + w0 * st->cfg.k : nullptr;
        HIP_TRY(launch_detector(st->plan.detector, p, s));
    }
    const int rc = enqueue_rescue(st, d_pcm, n_windows, d_sym, d_mag, s);
    return rc < 0 ? rc : (int)n_windows;
}

// Device staging of host-pointer calls: samples, and windows of symbols and
// magnitudes (the two also grow when magnitudes are first asked for).
int fskd::ensure_dev(demod_t *st, size_t samples, size_t windows, bool mags)
{
    HIP_TRY(st->d_in.reserve(samples, samples / 4 + 64));
    if (windows > st->d_sym.cap || (mags && !st->d_mag.p))
        HIP_TRY(reserve_outputs(st->d_sym, st->d_mag, windows, windows / 4 + 16, st->cfg.k));
    return DEMOD_OK;
}

bool fskd::is_device_ptr(const void *p)
{
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

int fskd::ensure_host(demod_t *st, size_t samples, size_t windows)
{
    HIP_TRY(st->h_in.reserve(samples));
    if (windows > st->h_sym.cap)
        HIP_TRY(reserve_outputs(st->h_sym, st->h_mag, windows, 0, st->cfg.k));
    return DEMOD_OK;
}

// Packet-sized calls (a 60 ms packet plus the carry is <= 3903 samples):
// mapped, coherent (uncached on the device) pinned buffers. The kernel's
// buffer loads read the samples over PCIe and its stores write the results
// back, so a call is one launch and one synchronize instead of an H2D copy, a
// launch, a D2H copy and the synchronize. The kernels' loads are bounded by
// the buffer descriptor's record count, so nothing past the call's samples is
// touched. If the runtime cannot map the memory the copy path below serves.
static constexpr size_t kZeroCopySamples = 1 << 14;   // 32 KiB: 16 windows at hop n

static int ensure_zero_copy(demod_t *st)
{
    if (st->zc) return st->zc;
    // measurement switch, read at the first such call (include/demod.h)
    if (std::getenv("FSKD_NO_ZERO_COPY")) return st->zc = -1;
    const size_t wmax = kZeroCopySamples / 8;  // hop >= 8
    const bool ok = st->z_in.reserve(kZeroCopySamples) == hipSuccess &&
                    st->z_sym.reserve(wmax) == hipSuccess &&
                    st->z_mag.reserve(wmax * st->cfg.k) == hipSuccess &&
                    ((uintptr_t)st->z_in.d & 15) == 0;
    if (!ok) (void)hipGetLastError();
    st->zc = ok ? 1 : -1;
    return st->zc;
}

static int run_host_zero_copy(demod_t *st, const int16_t *pcm, size_t n_samples, size_t n_windows,
                              uint8_t *symbols, float *mags)
{
    std::memcpy(st->z_in.p, pcm, n_samples * sizeof(int16_t));
    int rc = enqueue_batch(st, st->z_in.d, n_windows, st->z_sym.d, mags ? st->z_mag.d : nullptr,
                           st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipStreamSynchronize(st->stream));
    std::memcpy(symbols, st->z_sym.p, n_windows);
    if (mags) std::memcpy(mags, st->z_mag.p, n_windows * st->cfg.k * sizeof(float));
    return (int)n_windows;
}

// Small calls: one pinned round trip on one stream — 20 us per packet,
// against ~50 us through the chunked path's pageable copies and cross-stream
// events.
static int run_host_small(demod_t *st, const int16_t *pcm, size_t n_samples, size_t n_windows,
                          uint8_t *symbols, float *mags)
{
    int rc;
    if (n_samples <= kZeroCopySamples && ensure_zero_copy(st) == 1)
        return run_host_zero_copy(st, pcm, n_samples, n_windows, symbols, mags);
    if ((rc = ensure_dev(st, n_samples, n_windows, mags != nullptr)) != DEMOD_OK) return rc;
    if ((rc = ensure_host(st, kSmallHostSamples, kSmallHostSamples / 8)) != DEMOD_OK) return rc;
    if (pcm != st->h_in.p) std::memcpy(st->h_in.p, pcm, n_samples * sizeof(int16_t));
    HIP_TRY(hipMemcpyAsync(st->d_in.p, st->h_in.p, n_samples * sizeof(int16_t), hipMemcpyHostToDevice,
                           st->stream));
    rc = enqueue_batch(st, st->d_in.p, n_windows, st->d_sym.p, mags ? st->d_mag.p : nullptr, st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(st->h_sym.p, st->d_sym.p, n_windows, hipMemcpyDeviceToHost, st->stream));
    if (mags)
        HIP_TRY(hipMemcpyAsync(st->h_mag.p, st->d_mag.p, n_windows * st->cfg.k * sizeof(float),
                               hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    std::memcpy(symbols, st->h_sym.p, n_windows);
    if (mags) std::memcpy(mags, st->h_mag.p, n_windows * st->cfg.k * sizeof(float));
    return (int)n_windows;
}

// Large calls: the input goes to the device in chunks of kChunkWindows windows
// straight from the caller's (pageable) buffer — hipMemcpyAsync moves pageable
// memory at the PCIe rate (57 GB/s pinned vs 56.5 GB/s pageable measured), so
// a host-side staging copy would only add a memcpy — into two alternating
// device slots, so the kernel of chunk c runs while chunk c + 1 is in flight.
// Symbols and magnitudes land in device buffers and come back with one copy each.
static constexpr size_t kChunkWindows = 1 << 16;  // 128 MiB of input at n = hop = 1024

int fskd::run_host(demod_t *st, const int16_t *pcm, size_t n_samples, size_t n_windows,
                   uint8_t *symbols, float *mags)
{
    // windows <= samples / 8 (hop >= 8), so the pinned outputs always fit
    if (n_samples <= kSmallHostSamples)
        return run_host_small(st, pcm, n_samples, n_windows, symbols, mags);
    const size_t hop = st->cfg.hop, n = st->cfg.n;
    const size_t cw = std::min(n_windows, kChunkWindows);
    const size_t slot = (cw - 1) * hop + n;  // samples per device slot
    int rc;
    if ((rc = ensure_dev(st, 2 * slot, n_windows, mags != nullptr)) != DEMOD_OK) return rc;
    if (!st->copy_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&st->copy_stream, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(hipEventCreateWithFlags(&st->copied[b], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&st->consumed[b], hipEventDisableTiming));
        }
    }
    for (size_t w0 = 0, c = 0; w0 < n_windows; w0 += cw, ++c) {
        const int b = (int)(c & 1);
        const size_t nw = std::min(cw, n_windows - w0);
        const size_t ns = (nw - 1) * hop + n;
        int16_t *d = st->d_in.p + b * slot;
        if (c >= 2) HIP_TRY(hipStreamWaitEvent(st->copy_stream, st->consumed[b], 0));
        HIP_TRY(hipMemcpyAsync(d, pcm + w0 * hop, ns * sizeof(int16_t), hipMemcpyHostToDevice,
                               st->copy_stream));
        HIP_TRY(hipEventRecord(st->copied[b], st->copy_stream));
        HIP_TRY(hipStreamWaitEvent(st->stream, st->copied[b], 0));
        rc = enqueue_batch(st, d, nw, st->d_sym.p + w0, mags ? st->d_mag.p + w0 * st->cfg.k : nullptr,
                           st->stream);
        if (rc < 0) return rc;
        HIP_TRY(hipEventRecord(st->consumed[b], st->stream));
    }
    HIP_TRY(hipMemcpyAsync(symbols, st->d_sym.p, n_windows, hipMemcpyDeviceToHost, st->stream));
    if (mags)
        HIP_TRY(hipMemcpyAsync(mags, st->d_mag.p, n_windows * st->cfg.k * sizeof(float),
                               hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    return (int)n_windows;
}

// The argument checks the batch entry points share: 1 to go on, else the
// call's return value (0: no windows). Two orders differ between the calls
// and are part of the ABI's behaviour: demod_batch returns 0 for no windows
// before it looks at the alignment (empty_first), while the async calls
// refuse a misaligned pointer first; and the spectrum call (need_fft) answers
// DEMOD_UNIMPLEMENTED for a non-FFT handle before the size and alignment
// checks.
static int check_batch_args(const demod_t *st, const void *pcm, size_t n_windows, const void *symbols,
                            bool empty_first, bool need_fft)
{
    if (!st || (!pcm && n_windows) || (!symbols && n_windows)) return DEMOD_BAD_ARG;
    if (need_fft && st->plan.detector != kDetFft) return DEMOD_UNIMPLEMENTED;
    if (n_windows > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    if (empty_first && n_windows == 0) return 0;
    if (((uintptr_t)pcm & 15) != 0) return DEMOD_BAD_ARG;
    return n_windows ? 1 : 0;
}

extern "C" {

int demod_batch(demod_t *st, const int16_t *pcm, size_t n_windows, uint8_t *symbols, float *mags)
{
    const int go = check_batch_args(st, pcm, n_windows, symbols, true, false);
    if (go <= 0) return go;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    const size_t n_samples = (n_windows - 1) * st->cfg.hop + st->cfg.n;
    const bool din = is_device_ptr(pcm), dsym = is_device_ptr(symbols);
    const bool dmag = mags ? is_device_ptr(mags) : dsym;
    if (din && dsym && dmag) {
        int rc = enqueue_batch(st, pcm, n_windows, symbols, mags, st->stream);
        if (rc < 0) return rc;
        HIP_TRY(hipStreamSynchronize(st->stream));
        return rc;
    }
    if (!din && !dsym && !dmag) return run_host(st, pcm, n_samples, n_windows, symbols, mags);
    return DEMOD_BAD_ARG;  // mixed host/device pointers
}

int demod_batch_async(demod_t *st, const int16_t *d_pcm, size_t n_windows, uint8_t *d_symbols,
                      float *d_mags, void *stream)
{
    const int go = check_batch_args(st, d_pcm, n_windows, d_symbols, false, false);
    if (go <= 0) return go;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    return enqueue_batch(st, d_pcm, n_windows, d_symbols, d_mags, (hipStream_t)stream);
}

int demod_batch_spectrum_async(demod_t *st, const int16_t *d_pcm, size_t n_windows,
                               uint8_t *d_symbols, float *d_mags, float *d_spectrum, void *stream)
{
    const int go = check_batch_args(st, d_pcm, n_windows, d_symbols, false, true);
    if (go <= 0) return go;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    return enqueue_fft(st, d_pcm, n_windows, d_symbols, d_mags, d_spectrum, (hipStream_t)stream);
}

int demod_segments_layout(const demod_cfg_t *cfg, size_t n_segments, const size_t *n_samples,
                          uint64_t *first, uint32_t *count, size_t *n_windows)
{
    static_assert(sizeof(size_t) == sizeof(uint64_t), "run_layout writes first[] as size_t");
    if (validate_cfg(cfg) != DEMOD_OK || !n_samples || !n_windows) return DEMOD_BAD_ARG;
    if (n_segments == 0 || n_segments > DEMOD_MAX_SEGMENTS) return DEMOD_BAD_ARG;
    // a batch below 2^31 windows: refused before anything is written
    size_t W = 0;
    const auto total = [&](size_t s) { return n_samples[s]; };
    for (size_t s = 0; s < n_segments; ++s)
        if (n_samples[s] / cfg->hop > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    if (run_layout(n_segments, cfg->n, cfg->hop, total, nullptr, nullptr, &W) > 0x7FFFFFFF)
        return DEMOD_BAD_ARG;
    *n_windows = run_layout(n_segments, cfg->n, cfg->hop, total, reinterpret_cast<size_t *>(first),
                            count, &W);
    return DEMOD_OK;
}

int demodulate_mags(demod_t *st, const int16_t *pcm, size_t n_frames, uint8_t *symbols,
                    float *mags, size_t max_symbols)
{
    if (!st || (!pcm && n_frames)) return DEMOD_BAD_ARG;
    const demod_cfg_t &c = st->cfg;
    // lead-in (cfg.lead_in): the first frames of a stream are dropped, e.g. the
    // Opus decoder delay (OPUS_GET_LOOKAHEAD, 312 samples at 48 kHz for the
    // transmitter's settings, OpusEncoder.kt:65-67), so windows line up with
    // the transmitter's symbol boundaries
    const size_t drop = std::min(st->skip, n_frames);
    pcm += drop * c.channels;
    n_frames -= drop;
    const size_t have = st->carry.size();
    const size_t total = have + n_frames;
    const size_t W = windows_for(total, c.n, c.hop);
    if (W > max_symbols) return DEMOD_BUFFER_TOO_SMALL;
    if (W && !symbols) return DEMOD_BAD_ARG;
    if (W > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    // Mono view: carried samples followed by the new frames' selected channel.
    // Packet-sized calls (the playback.cpp:118 position: 2880 frames) build it
    // straight in the pinned staging buffer the small-call path copies from.
    int16_t *m = nullptr;
    if (W && total <= kSmallHostSamples) {
        int rc = ensure_host(st, kSmallHostSamples, kSmallHostSamples / 8);
        if (rc != DEMOD_OK) return rc;
        m = st->h_in.p;
    } else {
        st->scratch.resize(total);
        m = st->scratch.data();
    }
    if (have) std::memcpy(m, st->carry.data(), have * sizeof(int16_t));
    mono_frames(c, pcm, n_frames, m + have);
    if (W) {
        const size_t used = (W - 1) * c.hop + c.n;
        int rc = run_host(st, m, used, W, symbols, mags);
        if (rc < 0) return rc;  // nothing consumed on failure
    }
    const size_t consumed = W * c.hop;
    st->carry.assign(m + consumed, m + total);
    st->skip -= drop;
    return (int)W;
}

int demodulate(demod_t *st, const int16_t *pcm, size_t n_frames, uint8_t *symbols,
               size_t max_symbols)
{
    return demodulate_mags(st, pcm, n_frames, symbols, nullptr, max_symbols);
}

int demod_synth_fsk(const demod_cfg_t *cfg, uint64_t seed, uint64_t w0, size_t n_windows,
                    int amplitude, int sigma, int16_t *d_pcm, uint8_t *d_symbols, void *stream)
{
    if (!cfg || cfg->k < 1 || cfg->k > DEMOD_MAX_TONES || cfg->n < 8 || (cfg->n % 8)) return DEMOD_BAD_ARG;
    if (!(cfg->fs > 0.0) || !d_pcm || ((uintptr_t)d_pcm & 15)) return DEMOD_BAD_ARG;
    if (amplitude < 0 || amplitude > 32767 || sigma < 0 || sigma > 32767) return DEMOD_BAD_ARG;
    if (n_windows == 0) return DEMOD_OK;
    if (cfg->device < 0 || cfg->device >= kMaxDevices) return DEMOD_BAD_ARG;
    DeviceGuard guard(cfg->device);
    HIP_TRY(guard.err);
    // the buffers must live on cfg->device (the launch goes there)
    for (const void *q : {(const void *)d_pcm, (const void *)d_symbols}) {
        if (!q) continue;
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, q) != hipSuccess) {
            (void)hipGetLastError();
            continue;  // not a runtime allocation: left to the caller
        }
        if (a.type == hipMemoryTypeDevice && a.device != cfg->device) return DEMOD_BAD_ARG;
    }
    HIP_TRY(synth_prepare());  // sine table on the current device (once, locked)
    SynthParams p;
    std::memset(&p, 0, sizeof(p));
    p.seed = seed;
    p.w0 = w0;
    p.n_windows = (long long)n_windows;
    p.n = (int)cfg->n;
    p.k = (int)cfg->k;
    p.amplitude = amplitude;
    p.sigma = sigma;
    p.pcm = d_pcm;
    p.sym = d_symbols;
    for (uint32_t t = 0; t < cfg->k; ++t)
        p.inc[t] = (uint32_t)((unsigned long long)std::llround(cfg->freqs[t] / cfg->fs * 4294967296.0) &
                              0xFFFFFFFFULL);
    HIP_TRY(launch_synth(p, (hipStream_t)stream));
    return DEMOD_OK;
}

long long demod_frame_symbols_size(size_t n, int bits, size_t max_payload)
{
    if (bits < 1 || bits > 8) return DEMOD_BAD_ARG;
    if (max_payload < 1 || max_payload > DEMOD_MAX_FRAME_PAYLOAD) return DEMOD_BAD_ARG;
    if (n > (size_t)1 << 40) return DEMOD_BAD_ARG;
    return frame_streams_size((long long)n, bits, (long long)max_payload, nullptr, nullptr, nullptr);
}

long long demod_frame_streams_async(const uint8_t *d_symbols, size_t n_streams, size_t n,
                                    int bits, size_t max_payload, uint8_t *d_out, void *stream)
{
    const long long stride = demod_frame_symbols_size(n, bits, max_payload);
    if (stride < 0) return stride;
    if (n_streams && n && (!d_symbols || !d_out)) return DEMOD_BAD_ARG;
    if (n_streams > (size_t)1 << 31) return DEMOD_BAD_ARG;
    if (n_streams == 0 || n == 0) return stride;
    HIP_TRY(launch_frame_streams(d_symbols, (long long)n_streams, (long long)n, bits,
                                 (long long)max_payload, d_out, (hipStream_t)stream));
    return stride;
}

const char *demod_strerror(int error)
{
    switch (error) {
    case DEMOD_OK: return "success";
    case DEMOD_BAD_ARG: return "invalid argument";
    case DEMOD_BUFFER_TOO_SMALL: return "buffer too small";
    case DEMOD_INTERNAL_ERROR: return "internal error";
    case DEMOD_INVALID_PACKET: return "corrupted frame";
    case DEMOD_UNIMPLEMENTED: return "request not implemented";
    case DEMOD_INVALID_STATE: return "invalid state";
    case DEMOD_ALLOC_FAIL: return "memory allocation failed";
    case DEMOD_DEVICE_ERROR: return "HIP device error";
    case DEMOD_NO_DEVICE: return "no gfx950 (MI355X) device available";
    case DEMOD_FRAME_TOO_LARGE: return "encoded frame exceeds max size";
    default: return "unknown error";
    }
}

int demod_read_ceiling_async(const void *d_buf, size_t n_bytes, void *stream)
{
    if (!d_buf || ((uintptr_t)d_buf & 15) || (n_bytes % 8192)) return DEMOD_BAD_ARG;
    if (n_bytes == 0) return DEMOD_OK;
    HIP_TRY(launch_read_ceiling((const int16_t *)d_buf, (long long)n_bytes, (hipStream_t)stream));
    return DEMOD_OK;
}

const char *demod_version_string(void) { return "fskdemod 0.1.0 (gfx950 HIP)"; }

}  // extern "C"
