// demod_streams.cpp — many streams behind one detector handle (mono, the
// streams' n and hop). A push lays the streams' runs of complete windows end
// to end in one batch (stream_stage.h): one H2D copy of each run (the
// overlapping samples once), one detector launch (at hop = 64 H the
// segment-shared kernels, as a per-stream handle would run) and one D2H copy
// serve all streams.
#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "demod_host.h"
#include "stream_stage.h"

using namespace fskd;

static constexpr size_t kPushThreads = 8;  // demod_streams_push staging threads

// Persistent staging threads of one streams handle (the
// first build spawned and joined up to 7 std::threads inside every push).
// Workers sleep on a condition variable between pushes; run() hands worker k
// the stream range [k per, (k + 1) per), does range 0 on the calling thread
// and waits for the rest. A worker that cannot be started leaves its range
// to the caller.
struct StagePool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable go, done;
    const std::function<void(size_t, size_t)> *job = nullptr;
    size_t per = 0, S = 0, active = 0, pending = 0;
    unsigned long long gen = 0;
    bool stop = false;

    ~StagePool()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        go.notify_all();
        for (auto &t : th) t.join();
    }
    void worker(size_t k)
    {
        unsigned long long seen = 0;
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            go.wait(lk, [&] { return stop || gen != seen; });
            if (stop) return;
            seen = gen;
            if (k >= active) continue;
            const size_t a = k * per, e = std::min(S, a + per);
            const auto *f = job;
            lk.unlock();
            if (a < e) (*f)(a, e);
            lk.lock();
            if (--pending == 0) done.notify_one();
        }
    }
    // f(a, e) stages streams [a, e); T ranges in all (T - 1 on workers)
    void run(size_t T, size_t n, const std::function<void(size_t, size_t)> &f)
    {
        while (th.size() + 1 < T) {
            try {
                const size_t k = th.size() + 1;
                th.emplace_back([this, k] { worker(k); });
            } catch (...) {
                break;
            }
        }
        T = std::min(T, th.size() + 1);
        const size_t pr = (n + T - 1) / T;
        {
            std::lock_guard<std::mutex> lk(mu);
            job = &f;
            per = pr;
            S = n;
            active = T;
            pending = T - 1;
            ++gen;
        }
        if (T > 1) go.notify_all();
        f(0, std::min(n, pr));
        std::unique_lock<std::mutex> lk(mu);
        done.wait(lk, [&] { return pending == 0; });
        job = nullptr;
    }
    // f(s) for every stream s < n, on T ranges (T < 2: the calling thread)
    template <class F>
    void each(size_t T, size_t n, F f)
    {
        const std::function<void(size_t, size_t)> range = [&f](size_t a, size_t e) {
            for (size_t s = a; s < e; ++s) f(s);
        };
        if (T >= 2) run(T, n, range);
        else range(0, n);
    }
};

// A stream's mono samples not yet consumed by a complete window: < n of
// them, in a buffer of n that the first push allocates.
struct Carry {
    std::unique_ptr<int16_t[]> p;
    size_t len = 0;
    size_t have = 0;   // per push: len before it
};

struct demod_streams {
    demod_cfg_t cfg;                      // the streams' configuration
    demod_t *st = nullptr;                // detector handle: same n, hop, tones; mono
    std::vector<Carry> carry;
    std::vector<size_t> skip;             // lead-in frames still to drop per stream
    std::vector<size_t> first;            // per push: batch window of each stream's first
    std::vector<uint8_t> sym;             // per push: batch symbols / magnitudes
    std::vector<float> mag;
    std::vector<int16_t> dec;             // push_packets: [stream][frame_size x channels] decoded PCM
    std::vector<size_t> dec_frames;
    std::vector<const int16_t *> dec_ptr;
    StagePool pool;                       // staging threads of large pushes
    // FSKD_STREAMS_MAPPED=1 (measurement switch, read at create): the push
    // stages into mapped pinned memory that the detector reads in place over
    // PCIe and writes its results back to, instead of one H2D copy of the
    // staging buffer and a D2H copy of the results
    bool mapped = false;
    MappedBuf<int16_t> zm_in;             // samples
    MappedBuf<uint8_t> zm_sym;            // zm_sym.cap windows: zm_mag grows with it
    MappedBuf<float> zm_mag;
};

// Mapped staging of a push (demod_streams::mapped): samples and windows.
static int ensure_mapped(demod_streams_t *ms, size_t samples, size_t windows)
{
    HIP_TRY(ms->zm_in.reserve(samples, samples / 4 + 4096));
    if (windows > ms->zm_sym.cap)
        HIP_TRY(reserve_outputs(ms->zm_sym, ms->zm_mag, windows, windows / 4 + 64, ms->cfg.k));
    return DEMOD_OK;
}

// The samples stream s holds once a packet of n_frames frames has arrived.
static size_t stream_total(const demod_streams_t *ms, size_t s, size_t n_frames)
{
    return ms->carry[s].len + (n_frames > ms->skip[s] ? n_frames - ms->skip[s] : 0);
}

// Every refusal demod_streams_push makes from its arguments and the handle's
// state, before anything is consumed (all but the caller's cap and symbols
// buffer), and the symbols each stream will emit (exactly what the push
// writes to counts; nullable). demod_group.cpp runs it on every rank before
// the first collective, so a refusal is agreed on rather than met mid-protocol.
// Returns the total, or the push's negative code. The push itself also takes
// the batch layout it admits (stream_stage.h run_layout's first[] and Wb).
long long fskd::streams_check(const demod_streams_t *ms, const int16_t *const *pcm, const size_t *n_frames,
                              uint32_t *counts, size_t *first, size_t *Wb_out)
{
    if (!ms || !n_frames) return DEMOD_BAD_ARG;
    const size_t S = ms->carry.size(), n = ms->cfg.n, hop = ms->cfg.hop;
    for (size_t s = 0; s < S; ++s) {
        if (n_frames[s] && (!pcm || !pcm[s])) return DEMOD_BAD_ARG;
        if (n_frames[s] > ((size_t)1 << 40)) return DEMOD_BAD_ARG;
    }
    size_t W = 0;
    const size_t Wb = run_layout(S, n, hop, [&](size_t s) { return stream_total(ms, s, n_frames[s]); },
                                 first, counts, &W);
    if (W > 0x7FFFFFFF || W * n > ((size_t)1 << 40)) return DEMOD_BAD_ARG;
    // the batch also counts the straddling windows that are computed and
    // dropped, up to ~W n / hop: it must still fit an int count
    if (Wb > 0x7FFFFFFF || Wb * hop > ((size_t)1 << 40)) return DEMOD_BAD_ARG;
    if (Wb_out) *Wb_out = Wb;
    return (long long)W;
}

int fskd::streams_device(const demod_streams_t *ms) { return ms ? ms->st->device : -1; }

demod_t *fskd::streams_detector(demod_streams_t *ms) { return ms->st; }

size_t *fskd::streams_first(demod_streams_t *ms) { return ms->first.data(); }

void fskd::streams_copy_staging(demod_streams_t *ms) { ms->mapped = false; }

// stream s's fresh frames (past its lead-in) and where they start
static size_t fresh_frames(const demod_streams_t *ms, const size_t *n_frames, size_t s)
{
    return n_frames[s] - std::min(ms->skip[s], n_frames[s]);
}

static const int16_t *fresh_at(const demod_streams_t *ms, const int16_t *const *pcm, const size_t *n_frames,
                               size_t s, size_t f)
{
    return f ? pcm[s] + (n_frames[s] - f) * ms->cfg.channels : nullptr;
}

// The staging half of a push that streams_check admitted (W windows, Wb with
// the straddling ones, the layout in ms->first): every stream's carry and fresh
// frames to its run in the pinned staging buffer the host path copies from (or
// the mapped one), with room for `tail` more samples behind the runs, and the
// new carries formed. Until streams_commit the push can still be undone
// (streams_unstage). Returns DEMOD_OK or a code with nothing consumed.
int fskd::streams_stage(demod_streams_t *ms, const int16_t *const *pcm, const size_t *n_frames, size_t W,
                        size_t Wb, size_t tail, StreamsStage *out)
{
    const demod_cfg_t &c = ms->cfg;
    const size_t S = ms->carry.size(), n = c.n, hop = c.hop;
    demod_t *st = ms->st;
    // every carry holds < n samples after a push: n each, allocated once, so
    // the carry updates below never allocate
    for (Carry &cs : ms->carry) {
        if (!cs.p) cs.p.reset(new (std::nothrow) int16_t[n]);
        if (!cs.p) return DEMOD_ALLOC_FAIL;
        cs.have = cs.len;
    }
    out->W = W;
    out->Wb = Wb;
    out->samples = 0;
    out->base = nullptr;
    out->first = ms->first.data();
    if (!W && !tail) return DEMOD_OK;
    // (Wb, with the straddling windows, was bounded by streams_check)
    const int rc = ms->mapped ? ensure_mapped(ms, Wb * hop + n + tail, Wb)
                              : ensure_host(st, std::max(Wb * hop + n + tail, kSmallHostSamples),
                                            kSmallHostSamples / 8);
    if (rc != DEMOD_OK) return rc;
    out->base = ms->mapped ? ms->zm_in.p : st->h_in.p;
    if (!W) return DEMOD_OK;
    out->samples = (Wb - 1) * hop + n;  // the last run ends exactly here or earlier
    int16_t *const stage_base = out->base;
    // threads: ~1 per 2 MiB of staged samples, at most kPushThreads (1 per
    // MiB measured no better: 0.47 / 0.75 / 0.54-0.61 ms against 0.49-0.53 /
    // 0.67 / 0.55-0.59 for mono / stereo / hop 256 at 1024 streams); the
    // threads persist in the handle's pool between pushes
    const size_t T = std::min(std::min<size_t>(kPushThreads, Wb * hop / (1u << 20)), S);
    ms->pool.each(T, S, [&](size_t s) {
        const size_t f = fresh_frames(ms, n_frames, s);
        Carry &cs = ms->carry[s];
        cs.len = stage_stream(c, fresh_at(ms, pcm, n_frames, s, f), f, cs.p.get(), cs.have,
                              stage_base + ms->first[s] * hop);
    });
    return DEMOD_OK;
}

// The batch failed, nothing consumed: the carries come back from the staged runs.
void fskd::streams_unstage(demod_streams_t *ms, const size_t *n_frames, const StreamsStage &sg)
{
    if (!sg.W) return;
    for (size_t s = 0; s < ms->carry.size(); ++s) {
        Carry &cs = ms->carry[s];
        cs.len = unstage_stream(ms->cfg, fresh_frames(ms, n_frames, s), cs.p.get(), cs.have,
                                sg.base + ms->first[s] * ms->cfg.hop);
    }
}

// The batch succeeded: counts[s] = the windows stream s emitted (batch windows
// ms->first[s] ..), a stream without a complete window appends its frames to
// its carry, and the lead-ins are consumed.
void fskd::streams_commit(demod_streams_t *ms, const int16_t *const *pcm, const size_t *n_frames,
                          uint32_t *counts)
{
    const demod_cfg_t &c = ms->cfg;
    for (size_t s = 0; s < ms->carry.size(); ++s) {
        Carry &cs = ms->carry[s];
        const size_t f = fresh_frames(ms, n_frames, s), total = cs.have + f, w = windows_for(total, c.n, c.hop);
        counts[s] = (uint32_t)w;
        if (!w && f) {
            mono_frames(c, fresh_at(ms, pcm, n_frames, s, f), f, cs.p.get() + cs.have);  // total < n
            cs.len = total;
        }
        ms->skip[s] -= std::min(ms->skip[s], n_frames[s]);
    }
}

extern "C" {

demod_streams_t *demod_streams_create(const demod_cfg_t *cfg, size_t n_streams, int *error)
{
    demod_streams_t *ms = nullptr;
    const auto done = [&](int code) {   // a failure leaves nothing behind
        if (code != DEMOD_OK) demod_streams_destroy(ms);
        if (error) *error = code;
        return code != DEMOD_OK ? nullptr : ms;
    };
    int rc = validate_cfg(cfg);
    if (rc == DEMOD_OK && (n_streams < 1 || n_streams > ((size_t)1 << 24))) rc = DEMOD_BAD_ARG;
    if (rc != DEMOD_OK) return done(rc);
    ms = new (std::nothrow) demod_streams();
    if (!ms) return done(DEMOD_ALLOC_FAIL);
    ms->cfg = *cfg;
    demod_cfg_t dc = *cfg;
    dc.channels = 1;
    dc.channel_mode = DEMOD_CH_LEFT;
    dc.lead_in = 0;
    ms->st = demod_create(&dc, &rc);
    if (!ms->st) return done(rc);
    ms->mapped = ms->st->sw.streams_mapped;
    try {
        ms->carry.resize(n_streams);
        ms->skip.assign(n_streams, cfg->lead_in);
        ms->first.assign(n_streams, 0);
    } catch (...) {
        return done(DEMOD_ALLOC_FAIL);
    }
    return done(DEMOD_OK);
}

void demod_streams_destroy(demod_streams_t *ms)
{
    if (!ms) return;
    demod_destroy(ms->st);
    delete ms;
}

int demod_streams_reset(demod_streams_t *ms, size_t stream)
{
    if (!ms || stream >= ms->carry.size()) return DEMOD_BAD_ARG;
    ms->carry[stream].len = 0;
    ms->skip[stream] = ms->cfg.lead_in;
    return DEMOD_OK;
}

int demod_streams_pending(const demod_streams_t *ms, size_t stream)
{
    if (!ms || stream >= ms->carry.size()) return DEMOD_BAD_ARG;
    return (int)ms->carry[stream].len;
}

long long demod_streams_max_symbols(const demod_streams_t *ms, const size_t *n_frames)
{
    if (!ms || !n_frames) return DEMOD_BAD_ARG;
    long long w = 0;
    for (size_t s = 0; s < ms->carry.size(); ++s)
        w += (long long)windows_for(stream_total(ms, s, n_frames[s]), ms->cfg.n, ms->cfg.hop);
    return w;
}

int demod_streams_push(demod_streams_t *ms, const int16_t *const *pcm, const size_t *n_frames,
                       uint8_t *symbols, float *mags, size_t cap, uint32_t *counts)
{
    if (!ms || !n_frames || !counts) return DEMOD_BAD_ARG;
    const demod_cfg_t &c = ms->cfg;
    const size_t S = ms->carry.size();
    size_t Wb = 0;
    const long long Wc = streams_check(ms, pcm, n_frames, nullptr, ms->first.data(), &Wb);
    if (Wc < 0) return (int)Wc;
    const size_t W = (size_t)Wc;
    if (W > cap) return DEMOD_BUFFER_TOO_SMALL;
    if (W && !symbols) return DEMOD_BAD_ARG;
    demod_t *st = ms->st;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    if (W) {
        try {
            ms->sym.resize(Wb);
            if (mags) ms->mag.resize(Wb * c.k);
        } catch (...) {
            return DEMOD_ALLOC_FAIL;
        }
    }
    StreamsStage sg;
    int rc = streams_stage(ms, pcm, n_frames, W, Wb, 0, &sg);
    if (rc != DEMOD_OK) return rc;
    if (W) {
        if (ms->mapped) {
            // the detector reads the staged runs in place and writes the
            // results straight into mapped host memory: one launch (and the
            // rescue's), one synchronize
            rc = enqueue_batch(st, ms->zm_in.d, Wb, ms->zm_sym.d, mags ? ms->zm_mag.d : nullptr,
                               st->stream);
            if (rc >= 0 && hipStreamSynchronize(st->stream) != hipSuccess) rc = DEMOD_DEVICE_ERROR;
            if (rc >= 0) {
                std::memcpy(ms->sym.data(), ms->zm_sym.p, Wb);
                if (mags) std::memcpy(ms->mag.data(), ms->zm_mag.p, Wb * c.k * sizeof(float));
            }
        } else {
            rc = run_host(st, sg.base, sg.samples, Wb, ms->sym.data(), mags ? ms->mag.data() : nullptr);
        }
        if (rc < 0) {
            streams_unstage(ms, n_frames, sg);
            return rc;
        }
    }
    streams_commit(ms, pcm, n_frames, counts);
    uint8_t *so = symbols;
    float *mo = mags;
    for (size_t s = 0; s < S; ++s) {
        const size_t w = counts[s];
        if (!w) continue;
        std::memcpy(so, ms->sym.data() + ms->first[s], w);
        so += w;
        if (mags) {
            std::memcpy(mo, ms->mag.data() + ms->first[s] * c.k, w * c.k * sizeof(float));
            mo += w * c.k;
        }
    }
    return (int)W;
}

int demod_streams_push_packets(demod_streams_t *ms, demod_decode_fn decode, void *const *decoders,
                               const uint8_t *const *packets, const int32_t *lens, int frame_size,
                               uint8_t *symbols, float *mags, size_t cap, uint32_t *counts)
{
    if (!ms || !decode || !decoders || !lens || !counts) return DEMOD_BAD_ARG;
    if (frame_size < 1 || frame_size > (1 << 20)) return DEMOD_BAD_ARG;
    const size_t S = ms->carry.size(), ch = ms->cfg.channels, per = (size_t)frame_size * ch;
    for (size_t s = 0; s < S; ++s)
        if (lens[s] < 0 || (lens[s] > 0 && (!packets || !packets[s]))) return DEMOD_BAD_ARG;
    try {
        ms->dec.resize(S * per);
        ms->dec_frames.assign(S, 0);
        ms->dec_ptr.assign(S, nullptr);
    } catch (...) {
        return DEMOD_ALLOC_FAIL;
    }
    // every stream's packet decoded by its own decoder (playback.cpp:118,
    // opus_decode into the PCM buffer), on the handle's staging threads: the
    // decoders are independent, so are the streams. A zero-length packet is
    // no packet (playback.cpp:105 skips it): the stream pushes 0 frames.
    std::vector<int> err(S, 0);
    ms->pool.each(S < 8 ? 1 : std::min<size_t>(kPushThreads, S), S, [&](size_t s) {
        if (lens[s] == 0) return;
        int16_t *out = ms->dec.data() + s * per;
        const int got = decode(decoders[s], packets[s], lens[s], out, frame_size, 0);
        if (got < 0) err[s] = got;
        else if (got > frame_size) err[s] = DEMOD_INTERNAL_ERROR;   // the decoder overran its frame_size
        else {
            ms->dec_frames[s] = (size_t)got;
            ms->dec_ptr[s] = out;
        }
    });
    // the lowest stream's decode error: nothing pushed, no carry consumed
    // (the decoders' own states have advanced, as the reference's on a
    // failed opus_decode)
    for (size_t s = 0; s < S; ++s)
        if (err[s]) return err[s];
    return demod_streams_push(ms, ms->dec_ptr.data(), ms->dec_frames.data(), symbols, mags, cap, counts);
}

}  // extern "C"
