// demod_tx.cpp — the transmitter (include/demod.h "transmitter"): the shape
// check and the two device stages' entry points (frames_tx.hip), and the
// handle: frames in as demod_rx_push hands them out, samples out. The handle
// owns a detector handle (its device and stream), the ring, one device block
// places | states | samples with its pinned mirror, and the pinned staging of
// a send; a send is one copy in, encode and one copy out (places and states),
// a pull is the counts in, modulate and one copy out (states and samples).
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "demod_host.h"

using namespace fskd;

// What demod_tx_sizes refuses, and the launch parameters the shape decides.
static bool tx_shape(const demod_cfg_t *cfg, const demod_tx_cfg_t *x, size_t S, TxParams &p)
{
    if (!x || validate_cfg(cfg) != DEMOD_OK || cfg->k < 2) return false;
    const uint32_t K = cfg->k;
    if (x->sync_len < 1 || x->sync_len > DEMOD_MAX_SYNC || x->idle_len < 1 || x->idle_len > DEMOD_MAX_SYNC)
        return false;
    for (uint32_t i = 0; i < x->sync_len; ++i)
        if (x->sync[i] >= K) return false;
    for (uint32_t i = 0; i < x->idle_len; ++i)
        if (x->idle[i] >= K) return false;
    const uint32_t most = x->len_bytes == 1 ? 255u : (uint32_t)DEMOD_MAX_FRAME_PAYLOAD;
    if (x->max_len > most) return false;
    // A(max_len), or negative for an unknown len_bytes, crc or fec, or a coded mode with K no power of two
    const long long A = demod_tx_frame_symbol_count(x, K, x->max_len);
    if (A < 0) return false;
    const unsigned long long C = x->ring_symbols;
    if (C < (unsigned long long)A + x->gap) return false;
    if (!group_rows_ok(S, x->max_frames, false) || S * C > 0x7FFFFFFFull) return false;
    if (x->max_samples == 0 || x->max_samples % 8 != 0) return false;
    if ((unsigned long long)S * x->max_samples > 0x7FFFFFFFull) return false;
    if (x->amplitude < 0 || x->amplitude > 32767 || x->sigma < 0 || x->sigma > 32767) return false;

    p.n_streams = (unsigned)S;
    p.ring_symbols = x->ring_symbols;
    p.n = cfg->n;
    p.log2n = 0;
    while ((1u << p.log2n) < cfg->n) ++p.log2n;   // validate_cfg: n is a power of two
    p.bits = demod_bits_per_symbol(K);
    p.sync_len = x->sync_len;
    p.idle_len = x->idle_len;
    for (uint32_t i = 0; i < x->sync_len; ++i)
        p.sync4[i >> 4] |= (unsigned long long)x->sync[i] << ((i & 15) * 4);
    for (uint32_t i = 0; i < x->idle_len; ++i)
        p.idle4[i >> 4] |= (unsigned long long)x->idle[i] << ((i & 15) * 4);
    p.max_frames = x->max_frames;
    p.max_len = x->max_len;
    p.gap = x->gap;
    p.len_bytes = (int)x->len_bytes;
    p.crc_bytes = frame_crc_bytes((int)x->crc);
    p.fec = (int)rs_mode_conv(x->fec);
    p.parity = (int)rs_parity(x->fec);
    if (p.parity) {
        uint8_t g[RS_MAX_PARITY + 1];
        rs_generator((unsigned)p.parity, g);
        for (int i = 0; i < p.parity; ++i) p.rs_g8[i >> 3] |= (unsigned long long)g[i + 1] << ((i & 7) * 8);
    }
    fill_crc_fields(p, p.crc_bytes);   // as the check passes them
    for (uint32_t t = 0; t < K; ++t)
        p.inc[t] = (uint32_t)((unsigned long long)std::llround(cfg->freqs[t] / cfg->fs * 4294967296.0) &
                              0xFFFFFFFFULL);
    p.amplitude = x->amplitude;
    p.sigma = x->sigma;
    p.seed = x->seed;
    p.stride = x->max_samples;
    p.work_stride = (cfg->n - 1 + x->max_samples) / cfg->n + 2;
    return true;
}

extern "C" {

int demod_tx_sizes(const demod_cfg_t *cfg, const demod_tx_cfg_t *txcfg, size_t n_streams,
                   demod_tx_sizes_t *out)
{
    TxParams p;
    std::memset(&p, 0, sizeof(p));
    if (!out || !tx_shape(cfg, txcfg, n_streams, p)) return DEMOD_BAD_ARG;
    const size_t S = n_streams, rows = S * txcfg->max_frames;
    out->max_symbols = (uint64_t)demod_tx_frame_symbol_count(txcfg, cfg->k, txcfg->max_len);
    out->ring_bytes = S * (size_t)txcfg->ring_symbols;
    out->state_bytes = S * sizeof(demod_tx_stream_state_t);
    out->places_bytes = rows * sizeof(demod_tx_place_t);
    out->records_bytes = rows * sizeof(demod_tx_record_t);
    out->bodies_bytes = rows * txcfg->max_len;
    out->pcm_bytes = S * (size_t)txcfg->max_samples * sizeof(int16_t);
    out->modulate_work_bytes = S * (size_t)p.work_stride * sizeof(uint32_t);
    return DEMOD_OK;
}

size_t demod_tx_modulate_workspace_size(const demod_cfg_t *cfg, const demod_tx_cfg_t *txcfg,
                                        size_t n_streams)
{
    demod_tx_sizes_t z;
    return demod_tx_sizes(cfg, txcfg, n_streams, &z) == DEMOD_OK ? (size_t)z.modulate_work_bytes : 0;
}

int demod_tx_encode_async(demod_t *st, const demod_tx_cfg_t *txcfg, demod_tx_stream_state_t *d_state,
                          uint8_t *d_ring, const demod_tx_record_t *d_records, const uint32_t *d_count,
                          const uint8_t *d_bytes, size_t n_bytes, size_t n_streams,
                          demod_tx_place_t *d_place, void *stream)
{
    if (!st || !d_state || !d_ring || !d_records || !d_count || !d_place || (!d_bytes && n_bytes))
        return DEMOD_BAD_ARG;
    if (n_bytes > 0xFFFFFFFFull) return DEMOD_BAD_ARG;
    if (!aligned8(d_state, d_place) || !aligned4(d_records, d_count)) return DEMOD_BAD_ARG;
    TxParams p;
    std::memset(&p, 0, sizeof(p));
    if (!tx_shape(&st->cfg, txcfg, n_streams, p)) return DEMOD_BAD_ARG;
    p.state = d_state;
    p.ring = d_ring;
    p.records = d_records;
    p.count = d_count;
    p.bytes = d_bytes;
    p.n_bytes = (unsigned)n_bytes;
    p.place = d_place;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(launch_tx_encode(p, (hipStream_t)stream));
    return DEMOD_OK;
}

int demod_tx_modulate_async(demod_t *st, const demod_tx_cfg_t *txcfg, demod_tx_stream_state_t *d_state,
                            uint8_t *d_ring, const uint32_t *d_count, size_t n_streams,
                            int16_t *d_pcm, void *d_work, size_t work_bytes, void *stream)
{
    if (!st || !d_state || !d_ring || !d_count || !d_pcm || !d_work) return DEMOD_BAD_ARG;
    if (((uintptr_t)d_pcm & 15) != 0 || !aligned8(d_state) || !aligned4(d_count, d_work)) return DEMOD_BAD_ARG;
    TxParams p;
    std::memset(&p, 0, sizeof(p));
    if (!tx_shape(&st->cfg, txcfg, n_streams, p)) return DEMOD_BAD_ARG;
    if (work_bytes < n_streams * (size_t)p.work_stride * sizeof(uint32_t)) return DEMOD_BAD_ARG;
    p.state = d_state;
    p.ring = d_ring;
    p.count = d_count;
    p.pcm = d_pcm;
    p.work = static_cast<uint32_t *>(d_work);
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(synth_prepare());   // the sine table on this device (once, locked)
    p.lut = synth_lut_device();
    if (!p.lut) return DEMOD_DEVICE_ERROR;
    HIP_TRY(launch_tx_modulate(p, (hipStream_t)stream));
    return DEMOD_OK;
}

}  // extern "C"

// ---- the handle ----------------------------------------------------------------

struct demod_tx {
    demod_cfg_t cfg;
    demod_tx_cfg_t tx;
    demod_tx_sizes_t sz;
    size_t S = 0;
    demod_t *st = nullptr;               // the device and the stream
    DevBuf<uint8_t> d_ring;              // [S][C]
    DevBuf<unsigned char> d_work;        // modulate's
    // in: counts [S] | records [S][max_frames] | bytes, device and pinned host
    DevBuf<unsigned char> d_in;
    PinnedBuf<unsigned char> h_in;
    // out: places [S][max_frames] | states [S] | pad to 16 | samples [S][stride]
    DevBuf<unsigned char> d_out;
    PinnedBuf<unsigned char> h_out;
    std::vector<uint32_t> slot;          // per send: each frame's index inside its stream's group

    size_t records_off() const { return S * sizeof(uint32_t); }
    size_t bytes_off() const { return records_off() + (size_t)sz.records_bytes; }
    size_t in_bytes() const { return bytes_off() + (size_t)sz.bodies_bytes; }
    size_t states_off() const { return (size_t)sz.places_bytes; }
    size_t pcm_off() const { return (states_off() + (size_t)sz.state_bytes + 15) / 16 * 16; }
    size_t out_bytes() const { return pcm_off() + (size_t)sz.pcm_bytes; }
    demod_tx_stream_state_t *d_state() { return reinterpret_cast<demod_tx_stream_state_t *>(d_out.p + states_off()); }
    demod_tx_stream_state_t *h_state() const { return reinterpret_cast<demod_tx_stream_state_t *>(h_out.p + states_off()); }
    int16_t *d_pcm() { return reinterpret_cast<int16_t *>(d_out.p + pcm_off()); }
};

static int tx_allocate(demod_tx_t *tx)
{
    HIP_TRY(tx->d_ring.reserve((size_t)tx->sz.ring_bytes));
    HIP_TRY(hipMemset(tx->d_ring.p, 0, (size_t)tx->sz.ring_bytes));
    HIP_TRY(tx->d_work.reserve((size_t)tx->sz.modulate_work_bytes));
    HIP_TRY(tx->d_in.reserve(tx->in_bytes() + 1));
    HIP_TRY(tx->h_in.reserve(tx->in_bytes() + 1));
    HIP_TRY(tx->d_out.reserve(tx->out_bytes()));
    HIP_TRY(tx->h_out.reserve(tx->out_bytes()));
    HIP_TRY(hipMemset(tx->d_out.p, 0, tx->out_bytes()));
    std::memset(tx->h_out.p, 0, tx->out_bytes());
    return DEMOD_OK;
}

extern "C" {

demod_tx_t *demod_tx_create(const demod_cfg_t *cfg, const demod_tx_cfg_t *txcfg, size_t n_streams,
                            int *error)
{
    demod_tx_t *tx = nullptr;
    const auto done = [&](int code) {   // a failure leaves nothing behind
        if (code != DEMOD_OK) {
            demod_tx_destroy(tx);
            tx = nullptr;
        }
        if (error) *error = code;
        return tx;
    };
    demod_tx_sizes_t sz;
    int rc = demod_tx_sizes(cfg, txcfg, n_streams, &sz);
    if (rc != DEMOD_OK) return done(rc);
    tx = new (std::nothrow) demod_tx();
    if (!tx) return done(DEMOD_ALLOC_FAIL);
    tx->cfg = *cfg;
    tx->tx = *txcfg;
    tx->sz = sz;
    tx->S = n_streams;
    tx->st = demod_create(cfg, &rc);
    if (!tx->st) return done(rc);
    DeviceGuard guard(tx->st->device);
    if (guard.err != hipSuccess) return done(DEMOD_DEVICE_ERROR);
    return done(tx_allocate(tx));
}

void demod_tx_destroy(demod_tx_t *tx)
{
    if (!tx) return;
    demod_destroy(tx->st);
    delete tx;   // the buffers free themselves
}

int demod_tx_reset(demod_tx_t *tx, size_t stream)
{
    if (!tx || stream >= tx->S) return DEMOD_BAD_ARG;
    demod_t *st = tx->st;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(hipMemsetAsync(tx->d_state() + stream, 0, sizeof(demod_tx_stream_state_t), st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    std::memset(tx->h_state() + stream, 0, sizeof(demod_tx_stream_state_t));
    return DEMOD_OK;
}

int demod_tx_state(const demod_tx_t *tx, size_t stream, demod_tx_stream_state_t *state)
{
    if (!tx || !state || stream >= tx->S) return DEMOD_BAD_ARG;
    *state = tx->h_state()[stream];
    return DEMOD_OK;
}

int demod_tx_device_buffers(demod_tx_t *tx, const int16_t **d_pcm, const uint8_t **d_ring)
{
    if (!tx) return DEMOD_BAD_ARG;
    if (d_pcm) *d_pcm = tx->d_pcm();
    if (d_ring) *d_ring = tx->d_ring.p;
    return DEMOD_OK;
}

int demod_tx_send(demod_tx_t *tx, const demod_rx_frame_t *frames, size_t n, const uint8_t *bodies,
                  size_t n_bytes, demod_tx_place_t *place)
{
    if (!tx || (n && !frames)) return DEMOD_BAD_ARG;
    const size_t S = tx->S, mf = tx->tx.max_frames, M = tx->tx.max_len;
    if (n > S * mf) return DEMOD_BAD_ARG;
    uint32_t *count = reinterpret_cast<uint32_t *>(tx->h_in.p);
    demod_tx_record_t *rec = reinterpret_cast<demod_tx_record_t *>(tx->h_in.p + tx->records_off());
    uint8_t *bytes = tx->h_in.p + tx->bytes_off();
    try {
        tx->slot.resize(n);
    } catch (...) {
        return DEMOD_ALLOC_FAIL;
    }
    // refusals first: nothing is staged or queued for a list that is refused
    std::memset(count, 0, S * sizeof(uint32_t));
    for (size_t i = 0; i < n; ++i) {
        const demod_rx_frame_t &f = frames[i];
        if (f.stream >= S || count[f.stream] >= mf) return DEMOD_BAD_ARG;
        if (f.body > n_bytes || f.length > n_bytes - f.body || (f.length && !bodies)) return DEMOD_BAD_ARG;
        tx->slot[i] = count[f.stream]++;
    }
    // grouped stably by stream; the accepted lengths' bytes packed densely, in input order
    size_t used = 0;
    for (size_t i = 0; i < n; ++i) {
        const demod_rx_frame_t &f = frames[i];
        demod_tx_record_t &r = rec[f.stream * mf + tx->slot[i]];
        r.length = f.length;
        r.body = 0;
        if (f.length <= M) {   // a longer one comes back as DEMOD_TX_BAD_LENGTH; its bytes are not read
            r.body = (uint32_t)used;
            if (f.length) std::memcpy(bytes + used, bodies + f.body, f.length);
            used += f.length;
        }
    }
    demod_t *st = tx->st;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    const size_t in = tx->bytes_off() + used;
    HIP_TRY(hipMemcpyAsync(tx->d_in.p, tx->h_in.p, in, hipMemcpyHostToDevice, st->stream));
    demod_tx_place_t *d_place = reinterpret_cast<demod_tx_place_t *>(tx->d_out.p);
    const int rc = demod_tx_encode_async(
        st, &tx->tx, tx->d_state(), tx->d_ring.p,
        reinterpret_cast<const demod_tx_record_t *>(tx->d_in.p + tx->records_off()),
        reinterpret_cast<const uint32_t *>(tx->d_in.p), tx->d_in.p + tx->bytes_off(), used, S, d_place,
        st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(tx->h_out.p, tx->d_out.p, tx->states_off() + (size_t)tx->sz.state_bytes,
                           hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    const demod_tx_place_t *h_place = reinterpret_cast<const demod_tx_place_t *>(tx->h_out.p);
    int accepted = 0;
    for (size_t i = 0; i < n; ++i) {
        const demod_tx_place_t &pl = h_place[frames[i].stream * mf + tx->slot[i]];
        accepted += pl.status == DEMOD_TX_OK;
        if (place) place[i] = pl;
    }
    return accepted;
}

long long demod_tx_pull(demod_tx_t *tx, const size_t *n_frames, int16_t *const *pcm)
{
    if (!tx || !n_frames || !pcm) return DEMOD_BAD_ARG;
    const size_t S = tx->S, stride = tx->tx.max_samples;
    for (size_t s = 0; s < S; ++s)
        if (n_frames[s] > stride || (n_frames[s] && !pcm[s])) return DEMOD_BAD_ARG;
    uint32_t *count = reinterpret_cast<uint32_t *>(tx->h_in.p);
    long long total = 0;
    for (size_t s = 0; s < S; ++s) {
        count[s] = (uint32_t)n_frames[s];
        total += (long long)n_frames[s];
    }
    demod_t *st = tx->st;
    DeviceGuard guard(st->device);
    HIP_TRY(guard.err);
    HIP_TRY(hipMemcpyAsync(tx->d_in.p, tx->h_in.p, S * sizeof(uint32_t), hipMemcpyHostToDevice, st->stream));
    const int rc = demod_tx_modulate_async(st, &tx->tx, tx->d_state(), tx->d_ring.p,
                                           reinterpret_cast<const uint32_t *>(tx->d_in.p), S, tx->d_pcm(),
                                           tx->d_work.p, (size_t)tx->sz.modulate_work_bytes, st->stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(tx->h_out.p + tx->states_off(), tx->d_out.p + tx->states_off(),
                           tx->out_bytes() - tx->states_off(), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    const int16_t *h_pcm = reinterpret_cast<const int16_t *>(tx->h_out.p + tx->pcm_off());
    for (size_t s = 0; s < S; ++s)
        if (n_frames[s]) std::memcpy(pcm[s], h_pcm + s * stride, n_frames[s] * sizeof(int16_t));
    return total;
}

}  // extern "C"
