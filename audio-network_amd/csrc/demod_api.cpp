// demod_api.cpp — C ABI host layer of libfskdemod.so (include/demod.h).
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
static int ensure_dev(demod_t *st, size_t samples, size_t windows, bool mags)
{
    HIP_TRY(st->d_in.reserve(samples, samples / 4 + 64));
    if (windows > st->d_sym.cap || (mags && !st->d_mag.p))
        HIP_TRY(reserve_outputs(st->d_sym, st->d_mag, windows, windows / 4 + 16, st->cfg.k));
    return DEMOD_OK;
}

static bool is_device_ptr(const void *p)
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

// ---- acquisition (acquire.hip) -------------------------------------------

// R = n / hop when it divides and is at most DEMOD_MAX_PHASES, else 0 (n and
// hop are powers of two for every valid configuration, so R is one)
static uint32_t acquire_phases(const demod_cfg_t &c)
{
    if (c.hop == 0 || c.n % c.hop != 0) return 0;
    const uint32_t r = c.n / c.hop;
    return (r >= 1 && r <= DEMOD_MAX_PHASES && (r & (r - 1)) == 0) ? r : 0;
}

size_t demod_acquire_workspace_size(const demod_cfg_t *cfg)
{
    if (validate_cfg(cfg) != DEMOD_OK) return 0;
    // [kAcqMaxBlocks][R] doubles, then as many 64-bit first-match words
    return (size_t)2 * kAcqMaxBlocks * acquire_phases(*cfg) * sizeof(double);
}

// The handle's R when the shape and the sync word are acceptable, else 0.
// whole: the batch is acquired as one stream and needs R windows (a segment
// with fewer is an outcome of the segmented call, not a refusal).
static uint32_t acquire_check(const demod_t *st, size_t n_windows, const uint8_t *sync,
                              size_t sync_len, uint32_t max_errors, bool whole = true)
{
    if (!st) return 0;
    const uint32_t R = acquire_phases(st->cfg);
    if (R == 0 || (whole && n_windows < R) || n_windows > 0x7FFFFFFF) return 0;
    if (sync_len > DEMOD_MAX_SYNC || (sync_len && (!sync || max_errors >= sync_len))) return 0;
    for (size_t i = 0; i < sync_len; ++i)
        if (sync[i] >= st->cfg.k) return 0;
    return R;
}

int demod_acquire_async(demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                        size_t n_windows, const uint8_t *sync, size_t sync_len,
                        uint32_t max_errors, uint8_t *d_out, size_t cap,
                        demod_acquire_result_t *d_result, void *d_work, void *stream)
{
    if (!d_symbols || !d_mags || !d_result || !d_work) return DEMOD_BAD_ARG;
    const uint32_t R = acquire_check(st, n_windows, sync, sync_len, max_errors);
    if (R == 0) return DEMOD_BAD_ARG;
    if ((cap && !d_out) || ((uintptr_t)d_result & 7) != 0 || ((uintptr_t)d_work & 7) != 0)
        return DEMOD_BAD_ARG;
    AcquireParams p;
    std::memset(&p, 0, sizeof(p));
    for (size_t i = 0; i < sync_len; ++i) p.sync[i] = sync[i];
    p.sym = d_symbols;
    p.mag = d_mags;
    p.n_windows = (long long)n_windows;
    p.per_phase = (long long)(n_windows / R);
    p.phases = (int)R;
    p.k = (int)st->cfg.k;
    p.sync_len = (int)sync_len;
    p.max_errors = max_errors;
    p.cap = cap;
    p.out = d_out;
    p.res = d_result;
    p.part = static_cast<double *>(d_work);
    p.first = reinterpret_cast<unsigned long long *>(p.part + (size_t)kAcqMaxBlocks * R);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_acquire(p, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_acquire(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                  size_t sync_len, uint32_t max_errors, uint8_t *out, size_t cap,
                  demod_acquire_result_t *result)
{
    if (!pcm || !result || (cap && !out) || ((uintptr_t)pcm & 15) != 0) return DEMOD_BAD_ARG;
    const uint32_t R = acquire_check(st, n_windows, sync, sync_len, max_errors);
    if (R == 0) return DEMOD_BAD_ARG;   // before the detector runs
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    const size_t n_samples = (n_windows - 1) * st->cfg.hop + st->cfg.n;
    const bool din = is_device_ptr(pcm);
    int rc;
    if ((rc = ensure_dev(st, din ? 0 : n_samples, n_windows, true)) != DEMOD_OK) return rc;
    HIP_TRY(st->d_acq_work.reserve(demod_acquire_workspace_size(&st->cfg)));  // bytes
    HIP_TRY(st->d_acq_res.reserve(1));
    const size_t dcap = std::min(cap, n_windows / R + 1);  // n_out <= ceil(W / R)
    HIP_TRY(st->d_acq_out.reserve(dcap, dcap / 4 + 16));
    if (!din)
        HIP_TRY(hipMemcpyAsync(st->d_in.p, pcm, n_samples * sizeof(int16_t), hipMemcpyHostToDevice,
                               st->stream));
    rc = enqueue_batch(st, din ? pcm : st->d_in.p, n_windows, st->d_sym.p, st->d_mag.p, st->stream);
    if (rc < 0) return rc;
    rc = demod_acquire_async(st, st->d_sym.p, st->d_mag.p, n_windows, sync, sync_len, max_errors,
                             dcap ? st->d_acq_out.p : nullptr, dcap, st->d_acq_res.p,
                             st->d_acq_work.p, st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(result, st->d_acq_res.p, sizeof(*result), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    if (result->n_written)
        HIP_TRY(hipMemcpy(out, st->d_acq_out.p, result->n_written, hipMemcpyDeviceToHost));
    return (int)result->n_written;
}

// ---- segmented acquisition (acquire_segments.hip) --------------------------

size_t demod_acquire_segments_workspace_size(const demod_cfg_t *cfg, size_t max_segments,
                                             size_t max_windows)
{
    if (validate_cfg(cfg) != DEMOD_OK) return 0;
    const uint32_t R = acquire_phases(*cfg);
    if (R == 0 || max_segments == 0 || max_segments > DEMOD_MAX_SEGMENTS || max_windows > 0x7FFFFFFF)
        return 0;
    const size_t tiles = (max_windows + kAcqTile - 1) / kAcqTile + max_segments;
    return acquire_seg_header_bytes(max_segments) + tiles * acquire_seg_tile_bytes(R);
}

int demod_acquire_segments_async(demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                                 size_t n_windows, const uint64_t *d_first,
                                 const uint32_t *d_count, size_t n_segments, const uint8_t *sync,
                                 size_t sync_len, uint32_t max_errors, uint8_t *d_out, size_t cap,
                                 demod_acquire_result_t *d_results, void *d_work,
                                 size_t work_bytes, void *stream)
{
    if (!d_symbols || !d_mags || !d_results || !d_work || !d_first || !d_count) return DEMOD_BAD_ARG;
    const uint32_t R = acquire_check(st, n_windows, sync, sync_len, max_errors, false);
    if (R == 0 || n_segments == 0 || n_segments > DEMOD_MAX_SEGMENTS) return DEMOD_BAD_ARG;
    if ((cap && !d_out) || ((uintptr_t)d_results & 7) != 0 || ((uintptr_t)d_work & 7) != 0 ||
        ((uintptr_t)d_first & 7) != 0 || ((uintptr_t)d_count & 3) != 0)
        return DEMOD_BAD_ARG;
    const size_t need = demod_acquire_segments_workspace_size(&st->cfg, n_segments, n_windows);
    if (need == 0 || work_bytes < need) return DEMOD_BAD_ARG;
    const size_t head = acquire_seg_header_bytes(n_segments);
    const size_t budget = (work_bytes - head) / acquire_seg_tile_bytes(R);
    AcquireSegParams p;
    std::memset(&p, 0, sizeof(p));
    for (size_t i = 0; i < sync_len; ++i) p.sync[i] = sync[i];
    p.sym = d_symbols;
    p.mag = d_mags;
    p.seg_first = reinterpret_cast<const unsigned long long *>(d_first);
    p.seg_count = d_count;
    p.n_windows = (long long)n_windows;
    p.n_segments = (unsigned)n_segments;
    p.budget = (unsigned)std::min<size_t>(budget, 0xFFFFFFFFu);
    p.phases = (int)R;
    p.k = (int)st->cfg.k;
    p.sync_len = (int)sync_len;
    p.max_errors = max_errors;
    p.cap = cap;
    p.out = d_out;
    p.res = d_results;
    // the header: first'[S] (8 bytes each), then count', first tile and tiles
    // [S] and the call's total (4 bytes each); then the tiles' words
    unsigned char *w = static_cast<unsigned char *>(d_work);
    p.w_first = reinterpret_cast<unsigned long long *>(w);
    p.w_count = reinterpret_cast<unsigned *>(w + 8 * n_segments);
    p.w_tile0 = p.w_count + n_segments;
    p.w_tiles = p.w_tile0 + n_segments;
    p.w_total = p.w_tiles + n_segments;
    p.part = reinterpret_cast<double *>(w + head);
    p.first = reinterpret_cast<unsigned long long *>(p.part + (size_t)p.budget * R);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_acquire_segments(p, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_acquire_segments(demod_t *st, const int16_t *pcm, size_t n_windows,
                           const uint64_t *first, const uint32_t *count, size_t n_segments,
                           const uint8_t *sync, size_t sync_len, uint32_t max_errors,
                           uint8_t *out, size_t cap, demod_acquire_result_t *results)
{
    if (!pcm || !results || !first || !count || (cap && !out) || ((uintptr_t)pcm & 15) != 0)
        return DEMOD_BAD_ARG;
    const uint32_t R = acquire_check(st, n_windows, sync, sync_len, max_errors);
    if (R == 0 || n_segments == 0 || n_segments > DEMOD_MAX_SEGMENTS) return DEMOD_BAD_ARG;
    // the tables are host memory here: refuse what the kernels would clamp
    size_t longest = 0;
    unsigned long long tiles = 0, rows = 0;
    for (size_t s = 0; s < n_segments; ++s) {
        if (count[s] < R || first[s] > n_windows || count[s] > n_windows - first[s])
            return DEMOD_BAD_ARG;
        longest = std::max<size_t>(longest, count[s]);
        tiles += (count[s] + (size_t)kAcqTile - 1) / kAcqTile;
        rows += std::min<unsigned long long>(cap, count[s] / R + 1);
    }
    if (rows > 0x7FFFFFFF) return DEMOD_BAD_ARG;   // the return value is their sum at most
    // a workspace for every tile: ceil(cover / T) + S of them. Disjoint segments
    // fit cover = n_windows; overlapping ones may hold more tiles than the batch
    const unsigned long long cover = std::max<unsigned long long>(
        n_windows, tiles > n_segments ? (tiles - n_segments) * kAcqTile : 0);
    if (cover > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    const size_t work = demod_acquire_segments_workspace_size(&st->cfg, n_segments, (size_t)cover);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    const size_t n_samples = (n_windows - 1) * st->cfg.hop + st->cfg.n;
    const bool din = is_device_ptr(pcm);
    int rc;
    if ((rc = ensure_dev(st, din ? 0 : n_samples, n_windows, true)) != DEMOD_OK) return rc;
    HIP_TRY(st->d_seg_work.reserve(work));  // bytes
    HIP_TRY(st->d_seg_first.reserve(n_segments));
    HIP_TRY(st->d_seg_count.reserve(n_segments));
    HIP_TRY(st->d_seg_res.reserve(n_segments));
    const size_t dcap = std::min(cap, longest / R + 1);  // n_out <= ceil(count / R)
    HIP_TRY(st->d_seg_out.reserve(dcap * n_segments, 16));
    HIP_TRY(st->h_seg_out.reserve(dcap * n_segments));
    HIP_TRY(hipMemcpyAsync(st->d_seg_first.p, first, n_segments * sizeof(uint64_t),
                           hipMemcpyHostToDevice, st->stream));
    HIP_TRY(hipMemcpyAsync(st->d_seg_count.p, count, n_segments * sizeof(uint32_t),
                           hipMemcpyHostToDevice, st->stream));
    if (!din)
        HIP_TRY(hipMemcpyAsync(st->d_in.p, pcm, n_samples * sizeof(int16_t), hipMemcpyHostToDevice,
                               st->stream));
    rc = enqueue_batch(st, din ? pcm : st->d_in.p, n_windows, st->d_sym.p, st->d_mag.p, st->stream);
    if (rc < 0) return rc;
    rc = demod_acquire_segments_async(st, st->d_sym.p, st->d_mag.p, n_windows, st->d_seg_first.p,
                                      st->d_seg_count.p, n_segments, sync, sync_len, max_errors,
                                      dcap ? st->d_seg_out.p : nullptr, dcap, st->d_seg_res.p,
                                      st->d_seg_work.p, work, st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(results, st->d_seg_res.p, n_segments * sizeof(*results),
                           hipMemcpyDeviceToHost, st->stream));
    // the rows through pinned staging in the same pass, then each row's written
    // bytes to the caller's [S][cap]
    if (dcap)
        HIP_TRY(hipMemcpyAsync(st->h_seg_out.p, st->d_seg_out.p, dcap * n_segments,
                               hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    unsigned long long total = 0;
    for (size_t s = 0; s < n_segments; ++s) {
        const size_t nw = (size_t)results[s].n_written;
        if (nw) std::memcpy(out + s * cap, st->h_seg_out.p + s * dcap, nw);
        total += nw;
    }
    return (int)total;
}

// ---- frame scan (acquire_frames.hip) ---------------------------------------

size_t demod_frames_workspace_size(const demod_cfg_t *cfg, size_t max_windows)
{
    if (validate_cfg(cfg) != DEMOD_OK) return 0;
    const uint32_t R = acquire_phases(*cfg);
    if (R == 0 || max_windows > 0x7FFFFFFF) return 0;
    return frames_work_bytes((max_windows + kAcqTile - 1) / kAcqTile, R);
}

// The handle's R when a frame scan of these arguments is acceptable, else 0:
// what acquire_check refuses, no word, or a frame of 2^31 windows or more.
static uint32_t frames_check(const demod_t *st, size_t n_windows, const uint8_t *sync,
                             size_t sync_len, uint32_t max_errors, size_t frame_symbols,
                             size_t max_frames, bool whole = true)
{
    const uint32_t R = acquire_check(st, n_windows, sync, sync_len, max_errors, whole);
    if (R == 0 || sync_len == 0 || max_frames > 0x7FFFFFFF) return 0;
    if (frame_symbols > 0x7FFFFFFF || (sync_len + frame_symbols) * R > 0x7FFFFFFF) return 0;
    return R;
}

int demod_frames_async(demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                       size_t n_windows, const uint8_t *sync, size_t sync_len,
                       uint32_t max_errors, size_t frame_symbols, demod_frame_hit_t *d_hits,
                       uint8_t *d_payload, uint8_t *d_packed, size_t max_frames,
                       demod_frames_result_t *d_result, void *d_work, size_t work_bytes,
                       void *stream)
{
    if (!d_symbols || !d_mags || !d_result || !d_work) return DEMOD_BAD_ARG;
    const uint32_t R = frames_check(st, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames);
    if (R == 0) return DEMOD_BAD_ARG;
    if ((max_frames && !d_hits) || ((uintptr_t)d_hits & 7) != 0 || ((uintptr_t)d_result & 7) != 0 ||
        ((uintptr_t)d_work & 7) != 0)
        return DEMOD_BAD_ARG;
    const size_t need = demod_frames_workspace_size(&st->cfg, n_windows);
    if (need == 0 || work_bytes < need) return DEMOD_BAD_ARG;
    const size_t tiles = (n_windows + kAcqTile - 1) / kAcqTile;
    FramesParams p;
    std::memset(&p, 0, sizeof(p));
    for (size_t i = 0; i < sync_len; ++i) p.sync[i] = sync[i];
    p.sym = d_symbols;
    p.mag = d_mags;
    p.n_windows = (long long)n_windows;
    p.per_phase = (long long)(n_windows / R);
    p.frame_symbols = (long long)frame_symbols;
    p.phases = (int)R;
    p.k = (int)st->cfg.k;
    p.bits = demod_bits_per_symbol(st->cfg.k);
    p.sync_len = (int)sync_len;
    p.max_errors = max_errors;
    p.max_frames = max_frames;
    p.hits = d_hits;
    p.payload = d_payload;
    p.packed = d_packed;
    p.res = d_result;
    p.part = static_cast<double *>(d_work);
    p.tail = reinterpret_cast<unsigned long long *>(p.part + (size_t)kAcqMaxBlocks * R);
    p.offs = reinterpret_cast<unsigned *>(p.tail + (size_t)kAcqMaxBlocks * R);
    p.count = p.offs + (tiles + 1) / 2 * 2;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_frames(p, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_frames(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                 size_t sync_len, uint32_t max_errors, size_t frame_symbols,
                 demod_frame_hit_t *hits, uint8_t *payload, uint8_t *packed, size_t max_frames,
                 demod_frames_result_t *result)
{
    if (!pcm || !result || (max_frames && !hits) || ((uintptr_t)pcm & 15) != 0) return DEMOD_BAD_ARG;
    const uint32_t R = frames_check(st, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames);
    if (R == 0) return DEMOD_BAD_ARG;   // before the detector runs
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    const size_t n_samples = (n_windows - 1) * st->cfg.hop + st->cfg.n;
    const bool din = is_device_ptr(pcm);
    const size_t N = frame_symbols;
    const size_t B = (N * (size_t)demod_bits_per_symbol(st->cfg.k) + 7) / 8;
    int rc;
    if ((rc = ensure_dev(st, din ? 0 : n_samples, n_windows, true)) != DEMOD_OK) return rc;
    const size_t work = demod_frames_workspace_size(&st->cfg, n_windows);
    HIP_TRY(st->d_frm_work.reserve(work));  // bytes
    HIP_TRY(st->d_frm_res.reserve(1));
    // complete hits are starts on one phase whose frame fits: W / R + 1 bounds them
    const size_t dcap = std::min(max_frames, n_windows / R + 1);
    const bool want_payload = payload && N && dcap, want_packed = packed && N && dcap;
    HIP_TRY(st->d_frm_hits.reserve(dcap));
    if (want_payload) HIP_TRY(st->d_frm_payload.reserve(dcap * N));
    if (want_packed) HIP_TRY(st->d_frm_packed.reserve(dcap * B));
    if (!din)
        HIP_TRY(hipMemcpyAsync(st->d_in.p, pcm, n_samples * sizeof(int16_t), hipMemcpyHostToDevice,
                               st->stream));
    rc = enqueue_batch(st, din ? pcm : st->d_in.p, n_windows, st->d_sym.p, st->d_mag.p, st->stream);
    if (rc < 0) return rc;
    rc = demod_frames_async(st, st->d_sym.p, st->d_mag.p, n_windows, sync, sync_len, max_errors, N,
                            dcap ? st->d_frm_hits.p : nullptr,
                            want_payload ? st->d_frm_payload.p : nullptr,
                            want_packed ? st->d_frm_packed.p : nullptr, dcap, st->d_frm_res.p,
                            st->d_frm_work.p, work, st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(result, st->d_frm_res.p, sizeof(*result), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    // the device list was cut at dcap >= every possible n_hits or at max_frames
    const size_t nw = (size_t)result->n_written;
    if (nw) {
        HIP_TRY(hipMemcpy(hits, st->d_frm_hits.p, nw * sizeof(*hits), hipMemcpyDeviceToHost));
        if (want_payload) HIP_TRY(hipMemcpy(payload, st->d_frm_payload.p, nw * N, hipMemcpyDeviceToHost));
        if (want_packed) HIP_TRY(hipMemcpy(packed, st->d_frm_packed.p, nw * B, hipMemcpyDeviceToHost));
    }
    return (int)nw;
}

// ---- segmented frame scan (acquire_frames_segments.hip) ---------------------

size_t demod_frames_segments_workspace_size(const demod_cfg_t *cfg, size_t max_segments,
                                            size_t max_windows)
{
    if (validate_cfg(cfg) != DEMOD_OK) return 0;
    const uint32_t R = acquire_phases(*cfg);
    if (R == 0 || max_segments == 0 || max_segments > DEMOD_MAX_SEGMENTS || max_windows > 0x7FFFFFFF)
        return 0;
    const size_t tiles = (max_windows + kAcqTile - 1) / kAcqTile + max_segments;
    return acquire_seg_header_bytes(max_segments) + frames_seg_tiles_bytes(tiles, R);
}

int demod_frames_segments_async(demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                                size_t n_windows, const uint64_t *d_first, const uint32_t *d_count,
                                size_t n_segments, const uint8_t *sync, size_t sync_len,
                                uint32_t max_errors, size_t frame_symbols, demod_frame_hit_t *d_hits,
                                uint8_t *d_payload, uint8_t *d_packed, size_t max_frames,
                                demod_frames_result_t *d_results, void *d_work, size_t work_bytes,
                                void *stream)
{
    if (!d_symbols || !d_mags || !d_results || !d_work || !d_first || !d_count) return DEMOD_BAD_ARG;
    const uint32_t R =
        frames_check(st, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames, false);
    if (R == 0 || n_segments == 0 || n_segments > DEMOD_MAX_SEGMENTS) return DEMOD_BAD_ARG;
    if ((unsigned long long)n_segments * max_frames > 0x7FFFFFFFull) return DEMOD_BAD_ARG;
    if ((max_frames && !d_hits) || ((uintptr_t)d_hits & 7) != 0 || ((uintptr_t)d_results & 7) != 0 ||
        ((uintptr_t)d_work & 7) != 0 || ((uintptr_t)d_first & 7) != 0 || ((uintptr_t)d_count & 3) != 0)
        return DEMOD_BAD_ARG;
    const size_t need = demod_frames_segments_workspace_size(&st->cfg, n_segments, n_windows);
    if (need == 0 || work_bytes < need) return DEMOD_BAD_ARG;
    const size_t head = acquire_seg_header_bytes(n_segments);
    const size_t budget = std::min<size_t>(frames_seg_budget(work_bytes - head, R), 0xFFFFFFFFu);
    FrameSegParams q;
    std::memset(&q, 0, sizeof(q));
    AcquireSegParams &p = q.seg;
    for (size_t i = 0; i < sync_len; ++i) p.sync[i] = sync[i];
    p.sym = d_symbols;
    p.mag = d_mags;
    p.seg_first = reinterpret_cast<const unsigned long long *>(d_first);
    p.seg_count = d_count;
    p.n_windows = (long long)n_windows;
    p.n_segments = (unsigned)n_segments;
    p.budget = (unsigned)budget;
    p.phases = (int)R;
    p.k = (int)st->cfg.k;
    p.sync_len = (int)sync_len;
    p.max_errors = max_errors;
    // the header as demod_acquire_segments_async lays it out, then the tiles'
    // words: part and tail [B][R], count [B][R], offs [B]
    unsigned char *w = static_cast<unsigned char *>(d_work);
    p.w_first = reinterpret_cast<unsigned long long *>(w);
    p.w_count = reinterpret_cast<unsigned *>(w + 8 * n_segments);
    p.w_tile0 = p.w_count + n_segments;
    p.w_tiles = p.w_tile0 + n_segments;
    p.w_total = p.w_tiles + n_segments;
    p.part = reinterpret_cast<double *>(w + head);
    p.first = reinterpret_cast<unsigned long long *>(p.part + budget * R);
    q.count = reinterpret_cast<unsigned *>(p.first + budget * R);
    q.offs = q.count + (budget * R + 1) / 2 * 2;
    q.frame_symbols = (long long)frame_symbols;
    q.bits = demod_bits_per_symbol(st->cfg.k);
    q.max_frames = max_frames;
    q.hits = d_hits;
    q.payload = d_payload;
    q.packed = d_packed;
    q.res = d_results;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_frames_segments(q, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_frames_segments(demod_t *st, const int16_t *pcm, size_t n_windows, const uint64_t *first,
                          const uint32_t *count, size_t n_segments, const uint8_t *sync,
                          size_t sync_len, uint32_t max_errors, size_t frame_symbols,
                          demod_frame_hit_t *hits, uint8_t *payload, uint8_t *packed,
                          size_t max_frames, demod_frames_result_t *results)
{
    if (!pcm || !results || !first || !count || (max_frames && !hits) || ((uintptr_t)pcm & 15) != 0)
        return DEMOD_BAD_ARG;
    const uint32_t R = frames_check(st, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames);
    if (R == 0 || n_segments == 0 || n_segments > DEMOD_MAX_SEGMENTS) return DEMOD_BAD_ARG;
    // the tables are host memory here: refuse what the kernels would clamp
    size_t longest = 0;
    unsigned long long tiles = 0, rows = 0;
    for (size_t s = 0; s < n_segments; ++s) {
        if (count[s] < R || first[s] > n_windows || count[s] > n_windows - first[s])
            return DEMOD_BAD_ARG;
        longest = std::max<size_t>(longest, count[s]);
        tiles += (count[s] + (size_t)kAcqTile - 1) / kAcqTile;
        rows += std::min<unsigned long long>(max_frames, count[s] / R + 1);
    }
    if (rows > 0x7FFFFFFF) return DEMOD_BAD_ARG;   // the return value is their sum at most
    // complete hits are starts on one phase whose frame fits: count / R + 1 bounds them
    const size_t dcap = std::min(max_frames, longest / R + 1);
    if ((unsigned long long)n_segments * dcap > 0x7FFFFFFFull) return DEMOD_BAD_ARG;
    // a workspace for every tile (overlapping segments may hold more than the batch)
    const unsigned long long cover = std::max<unsigned long long>(
        n_windows, tiles > n_segments ? (tiles - n_segments) * kAcqTile : 0);
    if (cover > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    const size_t work = demod_frames_segments_workspace_size(&st->cfg, n_segments, (size_t)cover);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    const size_t n_samples = (n_windows - 1) * st->cfg.hop + st->cfg.n;
    const bool din = is_device_ptr(pcm);
    const size_t N = frame_symbols;
    const size_t B = (N * (size_t)demod_bits_per_symbol(st->cfg.k) + 7) / 8;
    const size_t n_rows = dcap * n_segments;
    const bool want_payload = payload && N && dcap, want_packed = packed && N && dcap;
    int rc;
    if ((rc = ensure_dev(st, din ? 0 : n_samples, n_windows, true)) != DEMOD_OK) return rc;
    HIP_TRY(st->d_seg_work.reserve(work));  // bytes
    HIP_TRY(st->d_seg_first.reserve(n_segments));
    HIP_TRY(st->d_seg_count.reserve(n_segments));
    HIP_TRY(st->d_fsg_res.reserve(n_segments));
    HIP_TRY(st->d_fsg_hits.reserve(n_rows));
    HIP_TRY(st->h_fsg_hits.reserve(n_rows));
    if (want_payload) {
        HIP_TRY(st->d_fsg_payload.reserve(n_rows * N));
        HIP_TRY(st->h_fsg_payload.reserve(n_rows * N));
    }
    if (want_packed) {
        HIP_TRY(st->d_fsg_packed.reserve(n_rows * B));
        HIP_TRY(st->h_fsg_packed.reserve(n_rows * B));
    }
    HIP_TRY(hipMemcpyAsync(st->d_seg_first.p, first, n_segments * sizeof(uint64_t),
                           hipMemcpyHostToDevice, st->stream));
    HIP_TRY(hipMemcpyAsync(st->d_seg_count.p, count, n_segments * sizeof(uint32_t),
                           hipMemcpyHostToDevice, st->stream));
    if (!din)
        HIP_TRY(hipMemcpyAsync(st->d_in.p, pcm, n_samples * sizeof(int16_t), hipMemcpyHostToDevice,
                               st->stream));
    rc = enqueue_batch(st, din ? pcm : st->d_in.p, n_windows, st->d_sym.p, st->d_mag.p, st->stream);
    if (rc < 0) return rc;
    rc = demod_frames_segments_async(st, st->d_sym.p, st->d_mag.p, n_windows, st->d_seg_first.p,
                                     st->d_seg_count.p, n_segments, sync, sync_len, max_errors, N,
                                     dcap ? st->d_fsg_hits.p : nullptr,
                                     want_payload ? st->d_fsg_payload.p : nullptr,
                                     want_packed ? st->d_fsg_packed.p : nullptr, dcap, st->d_fsg_res.p,
                                     st->d_seg_work.p, work, st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(results, st->d_fsg_res.p, n_segments * sizeof(*results),
                           hipMemcpyDeviceToHost, st->stream));
    // the rows through pinned staging in the same pass, then each segment's
    // written rows to the caller's [S][max_frames]
    if (dcap) {
        HIP_TRY(hipMemcpyAsync(st->h_fsg_hits.p, st->d_fsg_hits.p, n_rows * sizeof(*hits),
                               hipMemcpyDeviceToHost, st->stream));
        if (want_payload)
            HIP_TRY(hipMemcpyAsync(st->h_fsg_payload.p, st->d_fsg_payload.p, n_rows * N,
                                   hipMemcpyDeviceToHost, st->stream));
        if (want_packed)
            HIP_TRY(hipMemcpyAsync(st->h_fsg_packed.p, st->d_fsg_packed.p, n_rows * B,
                                   hipMemcpyDeviceToHost, st->stream));
    }
    HIP_TRY(hipStreamSynchronize(st->stream));
    unsigned long long total = 0;
    for (size_t s = 0; s < n_segments; ++s) {
        const size_t nw = (size_t)results[s].n_written;
        if (nw) {
            std::memcpy(hits + s * max_frames, st->h_fsg_hits.p + s * dcap, nw * sizeof(*hits));
            if (want_payload)
                std::memcpy(payload + s * max_frames * N, st->h_fsg_payload.p + s * dcap * N, nw * N);
            if (want_packed)
                std::memcpy(packed + s * max_frames * B, st->h_fsg_packed.p + s * dcap * B, nw * B);
        }
        total += nw;
    }
    return (int)total;
}

// ---- checked frames (frames_check.hip) ---------------------------------------

// Fills what the shape decides (row width, max_len, the CRC's constants, R,
// bits, L); false for what demod_frames_check_async refuses about it.
static bool frames_check_shape(const demod_t *st, size_t n_groups, size_t max_frames, size_t sync_len,
                               size_t frame_symbols, int len_bytes, int crc, FramesCheckParams &p,
                               int fec = 0)
{
    if (!st) return false;
    const uint32_t R = acquire_phases(st->cfg);
    if (R == 0 || n_groups == 0 || n_groups > DEMOD_MAX_SEGMENTS || max_frames == 0) return false;
    if (max_frames > 0x7FFFFFFF || (unsigned long long)n_groups * max_frames > 0x7FFFFFFFull) return false;
    if (sync_len == 0 || sync_len > DEMOD_MAX_SYNC || (len_bytes != 1 && len_bytes != 2)) return false;
    if (crc != DEMOD_CRC16_CCITT_FALSE && crc != DEMOD_CRC32_MPEG2) return false;
    const size_t bits = (size_t)demod_bits_per_symbol(st->cfg.k);
    const size_t c = crc == DEMOD_CRC16_CCITT_FALSE ? 2 : 4, h = (size_t)len_bytes;
    if (frame_symbols > 0x7FFFFFFF) return false;
    size_t B = (frame_symbols * bits + 7) / 8;
    if (fec) {
        // coded rows: St = floor(N bits / 2) steps decode to Bd = (St - 6) / 8 bytes
        const size_t St = frame_symbols * bits / 2;
        if (fec != DEMOD_FEC_CONV_K7 || st->cfg.k != (1u << bits)) return false;
        if (St < 8 * h + DEMOD_FEC_DEPTH) return false;
        B = (St - 6) / 8;
        p.fec_depth = DEMOD_FEC_DEPTH;
    }
    if (B < h + c || B - h - c > DEMOD_MAX_FRAME_PAYLOAD) return false;
    p.n_groups = (unsigned)n_groups;
    p.max_frames = (unsigned)max_frames;
    p.row_bytes = (unsigned)B;
    p.max_len = (unsigned)(B - h - c);
    p.len_bytes = len_bytes;
    p.crc_bytes = (int)c;
    p.poly = c == 2 ? 0x1021u << 16 : 0x04C11DB7u;
    p.init = c == 2 ? 0xFFFFu << 16 : 0xFFFFFFFFu;
    // x^8, then its squares mod P (Horner over the square's own coefficients, highest first)
    static_assert(DEMOD_MAX_FRAME_PAYLOAD + 2 < (1 << kCrcPowBits), "bytes after a lane's chunk");
    const int width = 8 * (int)c;
    p.xpow8[0] = 1u << (32 - width + 8);
    for (int j = 1; j < kCrcPowBits; ++j) {
        const uint32_t a = p.xpow8[j - 1];
        uint32_t r = 0, b = a;
        for (int i = 0; i < width; ++i, b <<= 1)
            r = (r << 1) ^ ((r >> 31) ? p.poly : 0u) ^ ((b >> 31) ? a : 0u);
        p.xpow8[j] = r;
    }
    p.bits = (int)bits;
    p.phases = (int)R;
    p.sync_len = (int)sync_len;
    return true;
}

// fec 0: the scan's packed rows; else decoded rows (the coded entry has refused fec 0)
static int frames_check_enqueue(demod_t *st, const demod_frame_hit_t *d_hits, const uint8_t *d_packed,
                                const demod_frames_result_t *d_results, size_t n_groups,
                                size_t max_frames, size_t sync_len, size_t frame_symbols, int len_bytes,
                                int crc, int fec, demod_frame_check_t *d_check, uint32_t *d_kept,
                                uint8_t *d_body, demod_frames_check_result_t *d_summary, void *stream)
{
    if (!st || !d_hits || !d_packed || !d_results || !d_check || !d_kept || !d_summary) return DEMOD_BAD_ARG;
    if (((uintptr_t)d_hits & 7) != 0 || ((uintptr_t)d_results & 7) != 0 || ((uintptr_t)d_summary & 7) != 0 ||
        ((uintptr_t)d_check & 3) != 0 || ((uintptr_t)d_kept & 3) != 0)
        return DEMOD_BAD_ARG;
    FramesCheckParams p;
    std::memset(&p, 0, sizeof(p));
    if (!frames_check_shape(st, n_groups, max_frames, sync_len, frame_symbols, len_bytes, crc, p, fec))
        return DEMOD_BAD_ARG;
    p.hits = d_hits;
    p.packed = d_packed;
    p.res = d_results;
    p.check = d_check;
    p.kept = d_kept;
    p.body = d_body;
    p.summary = d_summary;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_frames_check(p, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_frames_check_async(demod_t *st, const demod_frame_hit_t *d_hits, const uint8_t *d_packed,
                             const demod_frames_result_t *d_results, size_t n_groups,
                             size_t max_frames, size_t sync_len, size_t frame_symbols, int len_bytes,
                             int crc, demod_frame_check_t *d_check, uint32_t *d_kept, uint8_t *d_body,
                             demod_frames_check_result_t *d_summary, void *stream)
{
    return frames_check_enqueue(st, d_hits, d_packed, d_results, n_groups, max_frames, sync_len,
                                frame_symbols, len_bytes, crc, 0, d_check, d_kept, d_body, d_summary, stream);
}

// ---- coded frames (frames_fec.hip) -------------------------------------------

size_t demod_frames_decode_workspace_size(const demod_cfg_t *cfg, size_t n_groups, size_t max_frames,
                                          size_t frame_symbols)
{
    if (validate_cfg(cfg) != DEMOD_OK || cfg->k < 2 || (cfg->k & (cfg->k - 1)) != 0) return 0;
    if (n_groups == 0 || n_groups > DEMOD_MAX_SEGMENTS || max_frames == 0 || max_frames > 0x7FFFFFFF) return 0;
    if ((unsigned long long)n_groups * max_frames > 0x7FFFFFFFull) return 0;
    if (frame_symbols == 0 || frame_symbols > 0x7FFFFFFF) return 0;
    const size_t St = frame_symbols * (size_t)demod_bits_per_symbol(cfg->k) / 2;
    return n_groups * (size_t)fec_waves_per_group((unsigned)n_groups, (unsigned)max_frames) * St * 8;
}

int demod_frames_decode_async(demod_t *st, const demod_frame_hit_t *d_hits, const float *d_mags,
                              size_t n_windows, const uint64_t *d_first,
                              const demod_frames_result_t *d_results, size_t n_groups,
                              size_t max_frames, size_t sync_len, size_t frame_symbols, int len_bytes,
                              int crc, int fec, uint8_t *d_rows, demod_frame_decode_t *d_decode,
                              void *d_work, size_t work_bytes, void *stream)
{
    if (!st || !d_hits || !d_mags || !d_results || !d_rows || !d_decode || !d_work) return DEMOD_BAD_ARG;
    if (((uintptr_t)d_hits & 7) != 0 || ((uintptr_t)d_results & 7) != 0 || ((uintptr_t)d_work & 7) != 0 ||
        ((uintptr_t)d_first & 7) != 0 || ((uintptr_t)d_decode & 3) != 0)
        return DEMOD_BAD_ARG;
    if (fec != DEMOD_FEC_CONV_K7 || n_windows > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    FramesCheckParams q;   // the shape the coded check will see: the same refusals
    std::memset(&q, 0, sizeof(q));
    if (!frames_check_shape(st, n_groups, max_frames, sync_len, frame_symbols, len_bytes, crc, q, fec))
        return DEMOD_BAD_ARG;
    if ((sync_len + frame_symbols) * (size_t)q.phases > 0x7FFFFFFF) return DEMOD_BAD_ARG;
    const size_t need = demod_frames_decode_workspace_size(&st->cfg, n_groups, max_frames, frame_symbols);
    if (need == 0 || work_bytes < need) return DEMOD_BAD_ARG;
    FramesFecParams p;
    std::memset(&p, 0, sizeof(p));
    p.hits = d_hits;
    p.mag = d_mags;
    p.first = reinterpret_cast<const unsigned long long *>(d_first);
    p.res = d_results;
    p.n_windows = (unsigned)n_windows;
    p.n_groups = q.n_groups;
    p.max_frames = q.max_frames;
    p.frame_symbols = (unsigned)frame_symbols;
    p.steps = (unsigned)(frame_symbols * (size_t)q.bits / 2);
    p.row_bytes = q.row_bytes;
    p.max_len = q.max_len;
    p.len_bytes = q.len_bytes;
    p.crc_bytes = q.crc_bytes;
    p.k = (int)st->cfg.k;
    p.bits = q.bits;
    p.phases = q.phases;
    p.sync_len = q.sync_len;
    p.rows = d_rows;
    p.decode = d_decode;
    p.work = static_cast<unsigned long long *>(d_work);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_frames_decode(p, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_frames_check_coded_async(demod_t *st, const demod_frame_hit_t *d_hits, const uint8_t *d_rows,
                                   const demod_frames_result_t *d_results, size_t n_groups,
                                   size_t max_frames, size_t sync_len, size_t frame_symbols,
                                   int len_bytes, int crc, int fec, demod_frame_check_t *d_check,
                                   uint32_t *d_kept, uint8_t *d_body,
                                   demod_frames_check_result_t *d_summary, void *stream)
{
    if (fec != DEMOD_FEC_CONV_K7) return DEMOD_BAD_ARG;
    return frames_check_enqueue(st, d_hits, d_rows, d_results, n_groups, max_frames, sync_len,
                                frame_symbols, len_bytes, crc, fec, d_check, d_kept, d_body, d_summary, stream);
}

// demod_frames_checked (fec 0: the scan's packed rows) and demod_frames_coded
static int frames_checked_run(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                              size_t sync_len, uint32_t max_errors, size_t frame_symbols, int len_bytes,
                              int crc, int fec, demod_frame_hit_t *hits, uint32_t *lengths, uint8_t *body,
                              size_t max_frames, demod_frames_result_t *result,
                              demod_frames_check_result_t *summary)
{
    if (!pcm || !result || !summary || !hits || !lengths || ((uintptr_t)pcm & 15) != 0) return DEMOD_BAD_ARG;
    const uint32_t R = frames_check(st, n_windows, sync, sync_len, max_errors, frame_symbols, max_frames);
    if (R == 0) return DEMOD_BAD_ARG;   // before the detector runs
    // complete hits are starts on one phase whose frame fits: W / R + 1 bounds them
    const size_t dcap = std::min(max_frames, n_windows / R + 1);
    FramesCheckParams p;
    std::memset(&p, 0, sizeof(p));
    if (!frames_check_shape(st, 1, dcap, sync_len, frame_symbols, len_bytes, crc, p, fec)) return DEMOD_BAD_ARG;
    const size_t fec_work = fec ? demod_frames_decode_workspace_size(&st->cfg, 1, dcap, frame_symbols) : 0;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    const size_t n_samples = (n_windows - 1) * st->cfg.hop + st->cfg.n;
    const bool din = is_device_ptr(pcm);
    const size_t N = frame_symbols, B = p.row_bytes, M = p.max_len;
    const bool want_body = body && M;
    int rc;
    if ((rc = ensure_dev(st, din ? 0 : n_samples, n_windows, true)) != DEMOD_OK) return rc;
    const size_t work = demod_frames_workspace_size(&st->cfg, n_windows);
    HIP_TRY(st->d_frm_work.reserve(work));  // bytes
    HIP_TRY(st->d_frm_res.reserve(1));
    HIP_TRY(st->d_frm_hits.reserve(dcap));
    if (fec) {
        HIP_TRY(st->d_fec_rows.reserve(dcap * B));
        HIP_TRY(st->d_fec_decode.reserve(dcap));
        HIP_TRY(st->d_fec_work.reserve(fec_work));  // bytes
    } else {
        HIP_TRY(st->d_frm_packed.reserve(dcap * B));
    }
    HIP_TRY(st->d_chk_check.reserve(dcap));
    HIP_TRY(st->d_chk_kept.reserve(dcap));
    HIP_TRY(st->d_chk_sum.reserve(1));
    HIP_TRY(st->d_chk_hits.reserve(dcap));
    HIP_TRY(st->d_chk_len.reserve(dcap));
    if (want_body) HIP_TRY(st->d_chk_body.reserve(dcap * M));
    if (!din)
        HIP_TRY(hipMemcpyAsync(st->d_in.p, pcm, n_samples * sizeof(int16_t), hipMemcpyHostToDevice,
                               st->stream));
    rc = enqueue_batch(st, din ? pcm : st->d_in.p, n_windows, st->d_sym.p, st->d_mag.p, st->stream);
    if (rc < 0) return rc;
    rc = demod_frames_async(st, st->d_sym.p, st->d_mag.p, n_windows, sync, sync_len, max_errors, N,
                            st->d_frm_hits.p, nullptr, fec ? nullptr : st->d_frm_packed.p, dcap,
                            st->d_frm_res.p, st->d_frm_work.p, work, st->stream);
    if (rc < 0) return rc;
    if (fec) {
        rc = demod_frames_decode_async(st, st->d_frm_hits.p, st->d_mag.p, n_windows, nullptr, st->d_frm_res.p,
                                       1, dcap, sync_len, N, len_bytes, crc, fec, st->d_fec_rows.p,
                                       st->d_fec_decode.p, st->d_fec_work.p, fec_work, st->stream);
        if (rc < 0) return rc;
    }
    rc = frames_check_enqueue(st, st->d_frm_hits.p, fec ? st->d_fec_rows.p : st->d_frm_packed.p,
                              st->d_frm_res.p, 1, dcap, sync_len, N, len_bytes, crc, fec, st->d_chk_check.p,
                              st->d_chk_kept.p, want_body ? st->d_chk_body.p : nullptr, st->d_chk_sum.p,
                              st->stream);
    if (rc < 0) return rc;
    // the kept rows' hits and lengths side by side, so that only they cross to the host
    HIP_TRY(launch_frames_kept_rows(st->d_frm_hits.p, st->d_chk_check.p, st->d_chk_kept.p, st->d_chk_sum.p,
                                    (unsigned)dcap, st->d_chk_hits.p, st->d_chk_len.p, st->stream));
    HIP_TRY(hipMemcpyAsync(result, st->d_frm_res.p, sizeof(*result), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipMemcpyAsync(summary, st->d_chk_sum.p, sizeof(*summary), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    const size_t nk = (size_t)summary->n_kept;
    if (nk) {
        HIP_TRY(hipMemcpy(hits, st->d_chk_hits.p, nk * sizeof(*hits), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(lengths, st->d_chk_len.p, nk * sizeof(*lengths), hipMemcpyDeviceToHost));
        if (want_body) {
            // a body row holds its frame's bytes alone: the rest of the caller's row is left as it is
            st->h_chk_body.resize(nk * M);
            HIP_TRY(hipMemcpy(st->h_chk_body.data(), st->d_chk_body.p, nk * M, hipMemcpyDeviceToHost));
            for (size_t r = 0; r < nk; ++r)
                std::memcpy(body + r * M, st->h_chk_body.data() + r * M, lengths[r]);
        }
    }
    return (int)nk;
}

int demod_frames_checked(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                         size_t sync_len, uint32_t max_errors, size_t frame_symbols, int len_bytes,
                         int crc, demod_frame_hit_t *hits, uint32_t *lengths, uint8_t *body,
                         size_t max_frames, demod_frames_result_t *result,
                         demod_frames_check_result_t *summary)
{
    return frames_checked_run(st, pcm, n_windows, sync, sync_len, max_errors, frame_symbols, len_bytes, crc,
                              0, hits, lengths, body, max_frames, result, summary);
}

int demod_frames_coded(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                       size_t sync_len, uint32_t max_errors, size_t frame_symbols, int len_bytes,
                       int crc, int fec, demod_frame_hit_t *hits, uint32_t *lengths, uint8_t *body,
                       size_t max_frames, demod_frames_result_t *result,
                       demod_frames_check_result_t *summary)
{
    if (fec != DEMOD_FEC_CONV_K7) return DEMOD_BAD_ARG;
    return frames_checked_run(st, pcm, n_windows, sync, sync_len, max_errors, frame_symbols, len_bytes, crc,
                              fec, hits, lengths, body, max_frames, result, summary);
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
