/*
 * demod.h — C ABI of the MI355X acoustic-FSK demodulator (libfskdemod.so).
 *
 * This is the drop-in boundary for the north-star path.
 * The reference (tmarsteel/audio-network) has no demodulator; every entry
 * point below mirrors the shape of the C API that sits at the insertion
 * point in the reference receiver, right after `opus_decode`
 * (hardware/src/playback.cpp:118):
 *
 *   - an opaque handle created/destroyed like an Opus decoder
 *       opus_decoder_create / opus_decoder_destroy
 *       (hardware/lib/libopus/src/opus.h:423,512; playback.cpp:67-74);
 *   - caller-owned buffers, `int` return = count on success or a negative
 *     error code (opus_decode, opus.h:462; codes opus_defines.h:46-60);
 *   - errors are returned, never abort()ed (the reference call site aborts
 *     via OPUS_ERROR_CHECK, playback.cpp:16-22 — deliberately not copied);
 *   - frame bytes follow protocol/ip.proto:32-36,63-65 (ToReceiver{AudioData})
 *     with the varint32 length prefix of nanopb pb_encode_delimited /
 *     protobuf-java writeDelimitedTo (network.cpp:389-403,411;
 *     transmitter protobuf_async.kt:69-80,110-114).
 *
 * Threading: re-entrant across handles, not within one handle (one handle
 * serves one consumer, like the single playback task, playback.cpp:157-165).
 *
 * Decisions: every symbol is the argmax of the tone powers as the double-
 * precision definition computes them (ties to the lowest tone). The kernels
 * decide in fp32; a window whose fp32 top-2 margin lies within the powers'
 * error bound (derived from the kernel's operation sequence and constants,
 * demod_error_model) is flagged, and the decision rescue
 * decides it again in double and rewrites its symbol and powers: first by
 * 64-sample segments, or by the window folded to 128 samples where every
 * tone sits on a multiple of 8 bins, or by the residue fold (per tone the
 * 8-point DFT of the N/8-spaced samples at its residue b mod 8) for the
 * residue detector's integer-bin plans (n = 1024; each form with its own
 * derived bound against the definition's, so the rewritten powers are within
 * that bound of the definition's, not its bits; FSKD_PASS0_FOLD=0 keeps
 * segments), and where
 * that pass cannot decide, with the
 * definition's own arithmetic (powers bit-identical to it; every rescued
 * window with FSKD_RESCUE_SEG=0). The flag test runs in two stages: the int16 worst-case
 * energy first (no per-sample work), then, only for windows that test
 * flags, the window's own energy, so quiet input is not flagged wholesale.
 * The rescue runs inside the detector's own launch for every detector at
 * n = 1024 whose windows are evaluated one by one (plain bank, fold and FFT);
 * segment-shared windows (hop = 64 H < n, demod_slide_windows() > 0), the
 * residue detector's plans (their first pass lives there) and other window
 * lengths take a second launch on the same stream
 * (demod_batch_launches counts it). A batch is complete when its stream has
 * passed its launches; there is no state shared between batches, so batches
 * of one handle may run on different streams.
 *
 * Every compute entry point runs on the GPU (HIP, gfx950). There is no CPU
 * fallback: without a visible MI355X, demod_create() fails with
 * DEMOD_NO_DEVICE. The framing / packing helpers are pure host byte work.
 */
#ifndef FSKDEMOD_DEMOD_H
#define FSKDEMOD_DEMOD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (same numbering as opus_defines.h:46-60 where they overlap) */
#define DEMOD_OK                 0
#define DEMOD_BAD_ARG           -1  /* OPUS_BAD_ARG */
#define DEMOD_BUFFER_TOO_SMALL  -2  /* OPUS_BUFFER_TOO_SMALL */
#define DEMOD_INTERNAL_ERROR    -3  /* OPUS_INTERNAL_ERROR */
#define DEMOD_INVALID_PACKET    -4  /* OPUS_INVALID_PACKET: malformed frame bytes */
#define DEMOD_UNIMPLEMENTED     -5  /* OPUS_UNIMPLEMENTED */
#define DEMOD_INVALID_STATE     -6  /* OPUS_INVALID_STATE */
#define DEMOD_ALLOC_FAIL        -7  /* OPUS_ALLOC_FAIL */
#define DEMOD_DEVICE_ERROR      -8  /* a HIP runtime call failed */
#define DEMOD_NO_DEVICE         -9  /* no gfx950 device visible */
#define DEMOD_FRAME_TOO_LARGE  -10  /* payload > max encoded frame (network.cpp:24,223) */

#define DEMOD_MAX_TONES         16
/* Opus decoder delay of the transmitter's encoder settings at 48 kHz
 * (OPUS_GET_LOOKAHEAD; computed but never used by the reference,
 * transmitter OpusEncoder.kt:46-47,65-67; measured in SURVEY.md §8 a7). */
#define DEMOD_OPUS_LOOKAHEAD    312
#define DEMOD_MAX_FRAME_PAYLOAD 4096 /* MAX_ENCODED_FRAME_SIZE, network.cpp:24 */

/* channel handling for interleaved input (channels == 2) */
#define DEMOD_CH_LEFT     0   /* use channel 0 */
#define DEMOD_CH_RIGHT    1   /* use channel 1 */
#define DEMOD_CH_DOWNMIX  2   /* x = (L + R) >> 1 (arithmetic shift) */

/* detector selection */
#define DEMOD_METHOD_AUTO      0 /* FOLDED when eligible and k >= 3; else RESIDUE
                                    when eligible and k >= 5 (except overlapping
                                    windows at n = 1024, hop = 64 H <= 384, which
                                    take GOERTZEL); else GOERTZEL */
#define DEMOD_METHOD_GOERTZEL  1 /* per-window Goertzel tone bank over all n samples
                                    (n = 1024, hop = 64 H < n: 64-sample segments
                                    shared by the windows that contain them, same
                                    results as evaluating each window alone) */
#define DEMOD_METHOD_FFT       2 /* full-spectrum n-point real FFT (n = 1024), argmax
                                    over the tone bins round(f*n/fs); tones-only
                                    batches run the real split's post-pass only in
                                    the pair blocks holding a tone bin (same tone
                                    powers; demod_plan_info_t.fft_pmask;
                                    FSKD_FFT_PMASK=0 at demod_create: every block,
                                    a measurement switch) */
#define DEMOD_METHOD_FOLDED    3 /* Goertzel over the window folded to n/8 samples:
                                    exact when every tone is on a multiple of 8
                                    bins (f*n/fs integer, divisible by 8); at
                                    n = 1024, hop = 64 H < n the folded sums are
                                    carried from window to window (same results
                                    as evaluating each window alone).
                                    Magnitudes: its derived error bound implies
                                    |P_k - P_ref,k| <= 8.8e-6 P_max on an aligned
                                    window (north_star's 1e-5); the plain bank's
                                    (GOERTZEL, AUTO's choice at k <= 2) implies
                                    only 7e-5, so under AUTO configs[1]'s 1e-5
                                    magnitude bar is measured (every timed window,
                                    bench parity_all), not derived. FOLDED proves
                                    it at ~2 % of configs[1]'s step */
#define DEMOD_METHOD_RESIDUE   4 /* Goertzel over the window folded to n/8 samples per
                                    residue class of the bin mod 8: exact when every
                                    tone is on an integer bin (f*n/fs integer) */

typedef struct demod_cfg {
    double   fs;                     /* sample rate, Hz (48000) */
    uint32_t n;                      /* window length N in samples (1024) */
    uint32_t hop;                    /* window advance; == n for non-overlapping */
    uint32_t k;                      /* number of tones, 1..DEMOD_MAX_TONES */
    uint32_t channels;               /* 1 = mono, 2 = interleaved stereo */
    int32_t  channel_mode;           /* DEMOD_CH_* (ignored for mono) */
    int32_t  device;                 /* HIP device ordinal */
    int32_t  method;                 /* DEMOD_METHOD_* */
    uint32_t lead_in;                /* mono frames demodulate() drops at the start of a
                                        stream (after demod_create / demod_reset), e.g.
                                        DEMOD_OPUS_LOOKAHEAD to absorb the Opus decoder
                                        delay; 0 = none. < 2^31. Batch calls ignore it. */
    double   freqs[DEMOD_MAX_TONES]; /* tone frequencies, Hz; symbol i <-> freqs[i] */
} demod_cfg_t;

typedef struct demod demod_t;

/* Fill cfg with the 2-FSK defaults of SURVEY.md §8: fs 48 kHz, N = hop = 1024,
 * tones {1500, 3000} Hz, mono. */
void demod_cfg_default(demod_cfg_t *cfg);

/* Replaces opus_decoder_create (opus.h:423). NULL on failure, *error set. */
demod_t *demod_create(const demod_cfg_t *cfg, int *error);

/* Replaces opus_decoder_destroy (opus.h:512). NULL is accepted. */
void demod_destroy(demod_t *st);

/* Drop carried samples and re-arm cfg.lead_in; the next demodulate() starts a
 * new stream. Mirrors playback_start_new_stream (playback.cpp:67-74), which
 * recreates the Opus decoder (and with it its delay) per stream. */
int demod_reset(demod_t *st);

/* Detector the handle runs (DEMOD_METHOD_GOERTZEL / _FOLDED / _RESIDUE / _FFT). */
int demod_method(const demod_t *st);

/* Overlapping windows (n = 1024, hop = 64 H < n): the windows per tile the
 * detector's segment-shared kernel evaluates together (plain bank or fold,
 * DESIGN.md §4.8); 0 when every window is evaluated alone. The results are
 * the same either way. (FSKD_NO_SLIDE=1 in the environment at demod_create
 * turns the shared kernels off, for measurements.) */
int demod_slide_windows(const demod_t *st);

/* Number of mono samples currently carried between demodulate() calls. */
int demod_pending(const demod_t *st);

/* Upper bound on symbols the next demodulate(st, ., n_frames, ...) emits. */
int demod_max_symbols(const demod_t *st, size_t n_frames);

/* Kernel launches one device-pointer demod_batch / demod_batch_async of
 * n_windows makes (with_mags: magnitudes requested): the detector's, plus one
 * for the decision rescue where it is not inside the detector (K >= 2 on
 * segment-shared windows, residue plans or n != 1024; every other detector,
 * the FFT included, rescues inside its own launch). A Goertzel-family batch is one
 * detector launch; from 4 MiB of symbol + magnitude output it writes each
 * XCD's L2 back in a few bursts inside that launch instead of interleaving the
 * write-back with the input stream. With the environment
 * variable FSKD_WB_BURSTS=0 at demod_create (a measurement switch), batches
 * over ~10 MiB of output run as equal detector slices instead, and profilers
 * see that many dispatches. A host-pointer demod_batch over 4 MiB of samples
 * runs in chunks of 65 536 windows, each chunk counted as a batch of its own. */
int demod_batch_launches(const demod_t *st, size_t n_windows, int with_mags);

/* The decision rescue's threshold factor tau of this handle (0 when the
 * rescue is off, K = 1 or FSKD_NO_RESCUE=1): a window is re-decided in double
 * when its fp32 top-2 margin is below tau sqrt(NE P_max), NE the energy scale
 * of the window the detector transforms (n sum x^2; fold detector: (n/8)
 * sum xf^2 of the N/8-folded window, plus the oracle's share, see
 * demod_error_model_t.amb_d). tau = 4 (rho_det + rho_ref) / sqrt(n_eff) with
 * the bounds derived for the handle's tone plan and kernel (demod_error_model,
 * DESIGN.md §2a); no measured constant. For tests and diagnostics. */
double demod_rescue_tau(const demod_t *st);

/* The rescue's first pass (n = 1024: the Goertzel-family detectors, in the
 * kernel or, for segment-shared windows, in the rescue launch; and the FFT
 * detector's TONES-ONLY batches at its tone bins; a spectrum batch's flagged
 * windows always take the double FFT): a flagged window's powers in double by
 * 64-sample segments (fold plans and FFT plans whose tone bins are multiples
 * of 8: by the window folded to 128 samples) decide it when their top-2
 * margin clears tau64 sqrt(n sum x^2 P_max); windows inside that band take the
 * exact double chain (or double FFT). Returns tau64 = 4 rho_first / sqrt(n)
 * (0: every flagged window takes the exact path — n != 1024,
 * FSKD_RESCUE_SEG=0). For tests and diagnostics. */
double demod_rescue_tau64(const demod_t *st);

/* The error bounds behind the decision rescue, derived for a
 * configuration's tone plan from the kernel's operation sequence and fp32
 * constants by a forward rounding-error analysis; no device needed. For every
 * window x and tone k, with X_k the exact DFT of x at the tone (the fold /
 * residue / FFT detectors: at its bin):
 *   |sqrt(P_gpu,k) - |X_k||      <= rho_det sqrt(E_det)
 *   |sigma(P_oracle,k) - |X_k||  <= rho_ref sqrt(sum x^2)   sigma(P) = sign(P) sqrt|P|
 *   |sqrt(P_first,k) - sigma(P_oracle,k)| <= rho_first sqrt(sum x^2)  (pass 0)
 * E_det = sum x^2 of the window (plain bank, residue, FFT) or sum xf^2 of the
 * window folded to n/8 samples (energy = DEMOD_ENERGY_FOLDED). The kernels
 * flag a window when (P_1 - P_2)^2 < t2e E_eff P_1 (E_eff: the kernel's energy
 * E, Parseval's 2 sum_b P_b for the FFT (n sum x^2 from the samples on
 * tones-only batches that skip post-pass blocks), (sqrt E + amb_d)^2 for the fold
 * detector), which leaves unflagged only windows whose sqrt-power margin
 * exceeds twice the two bounds: their symbol is the oracle's. */
#define DEMOD_ENERGY_RAW      0
#define DEMOD_ENERGY_FOLDED   1
#define DEMOD_ENERGY_PARSEVAL 2
typedef struct demod_error_model {
    int32_t method;      /* the detector the configuration runs (DEMOD_METHOD_*) */
    int32_t energy;      /* DEMOD_ENERGY_*: the energy the kernel's flag test sums */
    double  rho_det;
    double  rho_ref;
    double  rho_first;   /* 0 when the configuration has no pass 0 (n != 1024, K = 1) */
    double  tau;         /* as demod_rescue_tau (0 for K = 1) */
    double  tau64;       /* as demod_rescue_tau64, before the handle's switches */
    double  t2e;         /* the stage-2 threshold factor the kernels read */
    double  t2e64;       /* pass 0's, with E its sum x^2 */
    double  amb_d;       /* fold detector: the oracle's share in units of sqrt(sum xf^2) */
} demod_error_model_t;
int demod_error_model(const demod_cfg_t *cfg, demod_error_model_t *model);

/* The tone plan a configuration runs and the fp32 constants its kernels read
 * (the arrays demod_create uploads), for operation-for-operation emulation in
 * tests; no device needed. rot receives rot_len float4 entries ([slot][g],
 * residue [slot][g][2]) when rot_cap (floats) allows, rot64 the first pass's
 * double tables ([k][16][4] then c[k]) when rot64_cap allows. */
typedef struct demod_plan_info {
    int32_t  method;        /* DEMOD_METHOD_* the configuration runs */
    int32_t  log2g;         /* lanes per window = 2^log2g = n / 64 */
    int32_t  reinsch;       /* plain bank: Reinsch-modified recurrence */
    int32_t  f16;           /* fold detector: fold by 16 (K = 8) */
    int32_t  dcls;          /* residue detector: compile-time class pattern */
    int32_t  slide;         /* segment-shared kernels (n = 1024, hop = 64 H < n) */
    uint64_t perm;          /* nibble s = the tone of kernel slot s (DCLS / F16) */
    int32_t  slot_tone[DEMOD_MAX_TONES];
    int32_t  zcls[DEMOD_MAX_TONES];
    int32_t  fft_bins[DEMOD_MAX_TONES];
    float    coef[DEMOD_MAX_TONES];
    float    sgn[DEMOD_MAX_TONES];
    double   rcoef[DEMOD_MAX_TONES];
    uint32_t rot_len;       /* float4 entries of rot */
    uint32_t rot64_len;     /* doubles of rot64 */
    int32_t  fold64;        /* pass 0's form: 1 = by the fold (rot64 rows are lane
                             * j's folded positions 8j .. 8j + 7 at the exact
                             * bins; fold detector plans), 2 = by the residue
                             * fold (residue detector plans, in the rescue
                             * launch), 0 = lane j's raw samples 64j .. */
    uint32_t fft_pmask;     /* FFT detector, tones only: bit jb = the real-split
                             * post-pass pair block jb (pairs 2jb, 2jb + 1 of
                             * every lane) holds a tone bin; only those blocks
                             * run (0xFF: all, the full spectrum's post-pass) */
} demod_plan_info_t;
int demod_plan_info(const demod_cfg_t *cfg, demod_plan_info_t *info, float *rot, size_t rot_cap,
                    double *rot64, size_t rot64_cap);

/*
 * Streaming entry point: demodulate(pcm, n) -> symbols.
 * pcm: host pointer to n_frames frames of `channels` interleaved int16
 * samples (48 kHz int16 LE, the format opus_decode writes at
 * playback.cpp:118). The stream's first cfg.lead_in frames are dropped; the
 * rest are appended to the handle's carry buffer;
 * one symbol is emitted per complete window (advance `hop`).
 * Returns the number of symbols written to symbols[0..], or a negative code.
 * If max_symbols is too small nothing is consumed and
 * DEMOD_BUFFER_TOO_SMALL is returned.
 * mags (nullable, host): receives k floats |X_k|^2 per emitted symbol.
 * Packet-sized calls (<= 16 Ki samples of carry + packet) run the kernel on
 * mapped, coherent pinned memory: one launch and one synchronize, no copies
 * (FSKD_NO_ZERO_COPY=1 in the environment at the handle's first such call
 * selects the copy path; a measurement switch, results are the same).
 */
int demodulate(demod_t *st, const int16_t *pcm, size_t n_frames,
               uint8_t *symbols, size_t max_symbols);
int demodulate_mags(demod_t *st, const int16_t *pcm, size_t n_frames,
                    uint8_t *symbols, float *mags, size_t max_symbols);

/*
 * Batch entry point (the GPU hot path): W windows of mono int16.
 * Window w starts at pcm + w * hop and is n samples long.
 * Pointers may be host or device memory (detected per call); the call is
 * synchronous. Returns W on success.
 */
int demod_batch(demod_t *st, const int16_t *pcm, size_t n_windows,
                uint8_t *symbols, float *mags);

/*
 * Asynchronous batch on a caller stream (hipStream_t passed as void*; NULL =
 * the HIP default stream, as in the HIP runtime API). All pointers must be
 * device pointers. Nothing is synchronised; returns W once enqueued.
 */
int demod_batch_async(demod_t *st, const int16_t *d_pcm, size_t n_windows,
                      uint8_t *d_symbols, float *d_mags, void *stream);

/*
 * Full-spectrum variant of demod_batch_async for DEMOD_METHOD_FFT handles:
 * additionally writes |X[b]|^2, b = 0..n/2, to d_spectrum[W][n/2 + 1]
 * (nullable). Other handles return DEMOD_UNIMPLEMENTED. Any float alignment
 * is accepted; a 16-byte-aligned d_spectrum takes the faster store path
 * (whole 16-byte stores of each 4-window group's rows).
 */
int demod_batch_spectrum_async(demod_t *st, const int16_t *d_pcm, size_t n_windows,
                               uint8_t *d_symbols, float *d_mags, float *d_spectrum,
                               void *stream);

/* ---- acquisition: symbol timing and sync word --------- */
/*
 * The detectors decide windows; with overlapping windows (hop < n) a batch
 * looks at the stream at every phase. Acquisition turns a batch's outputs,
 * sym[W] (uint8) and P[W][K] (fp32), window w at sample w hop, into the phase
 * on which symbols start, the window at which a frame starts, and the
 * symbol-rate stream after it. R = n / hop must divide exactly, 1 <= R <=
 * DEMOD_MAX_PHASES (n and hop are powers of two, so R is); W >= R;
 * J = floor(W / R).
 *
 *   phase metric  M[r] = sum_{j < J} (double) P[jR + r][sym[jR + r]], r < R:
 *                 the decided tone's power, summed in double. A symbol byte
 *                 >= K contributes nothing and its row of P is not read. The
 *                 tail windows w >= J R are left out, so every phase sums the
 *                 same count.
 *   phase         argmax_r M[r], ties to the lowest r.
 *   sync word     sync_len symbols (0 <= sync_len <= DEMOD_MAX_SYNC, each
 *                 < K; a HOST pointer, copied into the launch arguments, so a
 *                 captured graph bakes it in). For a start window w with
 *                 w + (sync_len - 1) R < W, errors(w) = #{i : sym[w + iR] !=
 *                 sync[i]} (a byte >= K mismatches). sync_window is the
 *                 lowest w = phase (mod R) with errors(w) <= max_errors, -1 if
 *                 there is none; sync_errors = errors(sync_window) (0 if
 *                 none). max_errors < sync_len is required.
 *   output        first_window = sync_window + sync_len R; phase when
 *                 sync_len == 0; W when a sync word was asked for and not
 *                 found. n_out = #{j >= 0 : first_window + jR < W}.
 *                 out[j] = sym[first_window + jR] for j < n_written =
 *                 min(n_out, cap); nothing is written past n_written.
 *
 * The sums' order depends on the shape (W, R) alone and no floating-point
 * atomic is used: results are bit-identical from run to run.
 */
#define DEMOD_MAX_PHASES   64
#define DEMOD_MAX_SYNC     64
#define DEMOD_ACQUIRE_TILE 1024   /* windows per workgroup tile of the scan */
typedef struct demod_acquire_result {
    double   metric[DEMOD_MAX_PHASES];  /* M[r], r < phases; the rest 0 */
    uint32_t phases, phase;
    uint64_t per_phase;                 /* J */
    int64_t  sync_window;               /* -1: none (or sync_len == 0) */
    uint32_t sync_errors, reserved;
    uint64_t first_window, n_out, n_written;
} demod_acquire_result_t;

/* Bytes of d_work an acquisition of this configuration needs (any W); 0 when
 * the configuration is invalid, n % hop != 0 or R > DEMOD_MAX_PHASES. No
 * device needed. */
size_t demod_acquire_workspace_size(const demod_cfg_t *cfg);

/*
 * Acquisition over a batch's device outputs, enqueued on `stream` (three short
 * launches; two when cap == 0). All d_* arguments are device pointers (d_work
 * and d_result 8-byte aligned); d_out may be NULL with cap 0. Nothing is
 * synchronised and nothing allocated, and the handle holds no state of it: the
 * caller owns d_work (demod_acquire_workspace_size bytes, contents arbitrary:
 * every word read is written first), so two acquisitions of one handle may run
 * on different streams, as batches may, and demod_batch_async followed by this
 * call can be captured into a HIP graph. Every byte of *d_result is written.
 * Returns DEMOD_OK once enqueued; DEMOD_BAD_ARG, before any launch, for
 * n % hop != 0, R > 64, W < R (or W >= 2^31), sync_len > 64, a sync symbol
 * >= K, max_errors >= sync_len when sync_len > 0, a NULL sync with sync_len
 * > 0, a NULL d_out with cap > 0, or a NULL d_symbols, d_mags, d_result or
 * d_work.
 */
int demod_acquire_async(demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                        size_t n_windows, const uint8_t *sync, size_t sync_len,
                        uint32_t max_errors, uint8_t *d_out, size_t cap,
                        demod_acquire_result_t *d_result, void *d_work, void *stream);

/*
 * The handle's detector over the n_windows sliding windows of pcm (a host or
 * device pointer, detected as demod_batch does), then the acquisition of its
 * outputs; out[0 .. n_written) and *result are copied to host memory.
 * Synchronous; uses the handle's own device buffers and a handle-owned
 * workspace allocated on first use. Returns n_written or a negative code.
 */
int demod_acquire(demod_t *st, const int16_t *pcm, size_t n_windows,
                  const uint8_t *sync, size_t sync_len, uint32_t max_errors,
                  uint8_t *out, size_t cap, demod_acquire_result_t *result);

/* ---- segmented acquisition: S segments of one batch in one call -------- */
/*
 * The acquisition above treats a batch as one stream whose timing never
 * moves. Here the batch holds S segments, segment s being batch windows
 * first[s] .. first[s] + count[s] - 1, and each is acquired exactly as a batch
 * of its own: with W = count[s] and window indices relative to first[s],
 * results[s] and out[s cap + j], j < n_written, are what the definitions above
 * give on (sym + first[s], P + first[s] K, count[s]); sync_window and
 * first_window are segment-relative, the tail w >= J R of a segment is left
 * out of its metric, and the sync word is compared only where
 * w + (sync_len - 1) R < count[s]: it never reads past its segment. Segments
 * that are the runs of many streams in one batch (demod_segments_layout) give
 * per-stream acquisition; consecutive blocks of one long stream give a phase
 * per block, so timing that moves (a dropped buffer, clock drift) is tracked.
 * Segments may touch, leave gaps, come in any order and overlap.
 *
 * d_first (uint64) and d_count (uint32) are DEVICE arrays, read when the
 * launches run: a captured graph may be replayed after they are rewritten in
 * place. The host never sees them, so the kernels clamp: first' = min(first,
 * n_windows), count' = min(count, n_windows - first'); no table content makes
 * them read outside the inputs or write outside the outputs and d_work.
 *
 * Short segments: a segment with count' < R reports phases = R, phase = 0,
 * per_phase = 0, metric all 0, sync_window = -1, sync_errors = 0,
 * first_window = count', n_out = n_written = 0 and writes nothing to out.
 *
 * Tile budget: the workspace stores per tile of DEMOD_ACQUIRE_TILE windows
 * (segment-relative; a segment of count' >= R windows has ceil(count' /
 * DEMOD_ACQUIRE_TILE) tiles, a shorter one none) and
 * demod_acquire_segments_workspace_size(cfg, S, Wmax) is a header for S
 * segments plus B = ceil(Wmax / DEMOD_ACQUIRE_TILE) + S tiles, which disjoint
 * segments of Wmax windows never exceed. A call's budget is the tiles its
 * work_bytes hold beyond the header for n_segments. Segment s is acquired
 * when the tiles of segments 0 .. s together are within the budget; the
 * others are reported as short segments are (first_window = count'). Callers
 * with overlapping segments size the workspace with a larger Wmax.
 *
 * Every sum's order depends on the segment's own (count', R): the same
 * contents at another first[s], in another slot or beside other segments give
 * bit-identical result and output bytes. No floating-point atomics.
 */
#define DEMOD_MAX_SEGMENTS 65536

/* Bytes of d_work for up to max_segments segments of a batch of up to
 * max_windows windows; monotone in both. 0 when the configuration is invalid
 * (as demod_acquire_workspace_size), max_segments is 0 or above
 * DEMOD_MAX_SEGMENTS, or max_windows >= 2^31. No device needed. */
size_t demod_acquire_segments_workspace_size(const demod_cfg_t *cfg, size_t max_segments,
                                             size_t max_windows);

/*
 * Enqueued on `stream`: four short launches whatever n_segments is (plan,
 * scan, finalise, gather; three when cap == 0). Nothing is allocated or
 * synchronised and the handle holds no state of the call; d_work may hold
 * anything on entry (every word read is written first by the same call).
 * d_out is [n_segments][cap] (NULL with cap 0); bytes of a row past its
 * n_written are not written. Every byte of d_results[0 .. n_segments) is.
 * Returns DEMOD_OK once enqueued; DEMOD_BAD_ARG, before any launch, for what
 * demod_acquire_async refuses except n_windows < R (a per-segment outcome
 * here), n_segments == 0 or > DEMOD_MAX_SEGMENTS, a NULL d_first or d_count,
 * work_bytes below demod_acquire_segments_workspace_size(cfg, n_segments,
 * n_windows), or a misaligned d_results, d_work, d_first (8 bytes) or d_count
 * (4 bytes).
 */
int demod_acquire_segments_async(demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                                 size_t n_windows, const uint64_t *d_first,
                                 const uint32_t *d_count, size_t n_segments, const uint8_t *sync,
                                 size_t sync_len, uint32_t max_errors, uint8_t *d_out, size_t cap,
                                 demod_acquire_result_t *d_results, void *d_work,
                                 size_t work_bytes, void *stream);

/*
 * The handle's detector over the n_windows sliding windows of pcm (a host or
 * device pointer, as demod_acquire), then the segmented acquisition of its
 * outputs. first, count, out ([n_segments][cap]; bytes of a row past its
 * n_written are left alone) and results are HOST memory. The tables are
 * checked here: a segment that leaves the batch or holds fewer than R windows
 * is refused with DEMOD_BAD_ARG before the detector runs. Synchronous;
 * handle-owned buffers grow on first use. Returns the sum of n_written or a
 * negative code.
 */
int demod_acquire_segments(demod_t *st, const int16_t *pcm, size_t n_windows,
                           const uint64_t *first, const uint32_t *count, size_t n_segments,
                           const uint8_t *sync, size_t sync_len, uint32_t max_errors,
                           uint8_t *out, size_t cap, demod_acquire_result_t *results);

/*
 * The batch layout demod_streams_push builds, for callers that hold S
 * recordings: run s of n_samples[s] mono samples has count[s] = its complete
 * windows, starts at batch window first[s] (sample first[s] hop of the batch)
 * and takes ceil(((count[s] - 1) hop + n) / hop) batch windows; the windows
 * between a run's last and the next run's first straddle two runs and belong
 * to no segment. *n_windows receives the batch's windows. first and count may
 * be NULL. Host only. DEMOD_OK, or DEMOD_BAD_ARG (an invalid configuration,
 * n_segments == 0 or > DEMOD_MAX_SEGMENTS, a batch of 2^31 windows or more).
 */
int demod_segments_layout(const demod_cfg_t *cfg, size_t n_segments, const size_t *n_samples,
                          uint64_t *first, uint32_t *count, size_t *n_windows);

/* ---- frame scan: every sync-word hit of a batch, with payloads ---------- */
/*
 * The acquisition above stops at the lowest window where the sync word
 * matches. A recording holds many frames; the frame scan makes the same phase
 * decision (R, J, M[r], phase and errors(w) exactly as "acquisition" defines
 * them; metric, phases, phase and per_phase come out byte-identical to
 * demod_acquire_async's on the same inputs) and then lists ALL hits on that
 * phase, each with a fixed-length payload.
 *
 *   L = sync_len, 1 <= L <= DEMOD_MAX_SYNC (the word a HOST pointer, copied
 *   into the launch arguments); max_errors < L; N = frame_symbols >= 0 payload
 *   symbols after the word, (L + N) R < 2^31; bits = demod_bits_per_symbol(K).
 *
 *   hit          a start w = phase (mod R) with w + (L - 1) R < W and
 *                errors(w) <= max_errors.
 *   complete     a hit with w + (L + N - 1) R < W: word and payload lie inside
 *                the batch (N = 0: the word itself is the frame).
 *   hits         the complete hits in ascending w; n_hits their number;
 *                n_written = min(n_hits, max_frames).
 *   tail_window  the lowest hit that is NOT complete (its frame runs past the
 *                batch's end), -1 if there is none; tail_errors its error
 *                count (0 if none).
 *
 * For i < n_written only:
 *   d_hits[i]    = {window_i, errors(window_i), 0}
 *   d_payload[i N + j] = sym[window_i + (L + j) R], j < N (raw bytes, a byte
 *                >= K included); may be NULL.
 *   d_packed[i B .. (i + 1) B), B = ceil(N bits / 8): what
 *                demod_pack_symbols(payload_i, N, bits, ..) writes (MSB first,
 *                each symbol masked to `bits` bits, pad bits 0); may be NULL.
 * Rows >= n_written and bytes outside these arrays are not written.
 *
 * Overlaps are reported, not resolved: a hit inside another frame's payload is
 * listed like any other, so `hits` is NOT a list of disjoint frames. Random
 * symbols hold the word at a rate of about C(L, <= max_errors) / K^L per
 * start, and a greedy hold-off is serial in the worst case; callers settle it
 * with the frame's own header or CRC ("checked frames" below does it on the
 * device for one frame format).
 *
 * Streaming: a caller that keeps its samples from tail_window on (or, with
 * tail_window == -1, from the first start on the phase whose word no longer
 * fits, w + (L - 1) R >= W) and puts them in front of the next batch loses no
 * frame.
 *
 * All output bytes are a function of the inputs alone (no floating-point
 * atomics, no atomics that decide a position): bit-identical from run to run
 * and stream to stream.
 */
typedef struct demod_frame_hit {
    uint64_t window;                    /* the word's first window */
    uint32_t errors, reserved;          /* errors(window); 0 */
} demod_frame_hit_t;

typedef struct demod_frames_result {
    double   metric[DEMOD_MAX_PHASES];  /* as demod_acquire_result_t */
    uint32_t phases, phase;
    uint64_t per_phase;
    uint64_t n_hits, n_written;
    int64_t  tail_window;               /* -1: none */
    uint32_t tail_errors, reserved;
} demod_frames_result_t;

/* Bytes of d_work a frame scan of up to max_windows windows needs; monotone in
 * max_windows. With T = ceil(max_windows / DEMOD_ACQUIRE_TILE) tiles: two
 * 8-byte words per phase for each of 1024 workgroups (16 * 1024 * R), one
 * 4-byte prefix per tile (4 T) and one 4-byte hit count per tile and phase
 * (4 T R), each rounded up to 8. 0 when the configuration is invalid, n % hop != 0,
 * R > DEMOD_MAX_PHASES or max_windows >= 2^31. No device needed. */
size_t demod_frames_workspace_size(const demod_cfg_t *cfg, size_t max_windows);

/*
 * The frame scan over a batch's device outputs, enqueued on `stream`: four
 * launches whatever the hit count is (scan, finalise, emit, gather; three when
 * d_payload and d_packed are both NULL or N == 0; two when max_frames == 0,
 * which is legal and counts only). All d_* arguments are device pointers
 * (d_hits, d_result and d_work 8-byte aligned; d_payload and d_packed at any
 * alignment). Nothing is allocated or synchronised and the handle keeps no
 * state of the call; d_work may hold anything on entry (every word a launch
 * reads is stored by an earlier launch of the same call), so the call can be
 * captured into a HIP graph behind demod_batch_async. Every byte of *d_result
 * is written. Returns DEMOD_OK once enqueued; DEMOD_BAD_ARG, before any
 * launch, for everything demod_acquire_async refuses (W < R included),
 * sync_len == 0, (L + N) R >= 2^31, a NULL d_hits with max_frames > 0,
 * max_frames >= 2^31, work_bytes below demod_frames_workspace_size(cfg,
 * n_windows), or a misaligned d_hits, d_result or d_work.
 */
int demod_frames_async(demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                       size_t n_windows, const uint8_t *sync, size_t sync_len,
                       uint32_t max_errors, size_t frame_symbols, demod_frame_hit_t *d_hits,
                       uint8_t *d_payload, uint8_t *d_packed, size_t max_frames,
                       demod_frames_result_t *d_result, void *d_work, size_t work_bytes,
                       void *stream);

/*
 * The handle's detector over the n_windows sliding windows of pcm (a host or
 * device pointer, as demod_acquire), then the frame scan of its outputs.
 * hits[max_frames], payload[max_frames][N] and packed[max_frames][B] (either
 * may be NULL) and *result are HOST memory; rows past n_written are left
 * alone. Synchronous; handle-owned buffers grow on first use. Returns
 * n_written or a negative code.
 */
int demod_frames(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                 size_t sync_len, uint32_t max_errors, size_t frame_symbols,
                 demod_frame_hit_t *hits, uint8_t *payload, uint8_t *packed, size_t max_frames,
                 demod_frames_result_t *result);

/* ---- segmented frame scan: every frame of every segment, one call ------- */
/*
 * The frame scan above picks ONE phase for the batch and lists the hits on it:
 * many streams in one batch, or a stream whose timing slips, lose frames. Here
 * the batch holds S segments, segment s being batch windows first[s] ..
 * first[s] + count[s] - 1 (the tables of "segmented acquisition": device
 * arrays read when the launches run, clamped first' = min(first, n_windows),
 * count' = min(count, n_windows - first'); segments may touch, leave gaps,
 * come in any order and overlap), and each is scanned exactly as a batch of
 * its own: with W = count'[s] and window indices relative to first'[s], the
 * "frame scan" definitions on (sym + first', P + first' K, count') give
 * results[s] and, for i < results[s].n_written,
 *
 *   d_hits[s max_frames + i]            (window segment-relative, as sync_window)
 *   d_payload[(s max_frames + i) N + j] (j < N)
 *   d_packed[(s max_frames + i) B ..)   (B = ceil(N bits / 8))
 *
 * A word or a payload never reads past its segment: a hit whose payload would
 * leave the segment is not complete and is that segment's tail_window. Rows
 * >= n_written of a segment are not written; every byte of d_results[0 .. S)
 * is. No table content makes the kernels read outside the inputs or write
 * outside the outputs and d_work.
 *
 * Short segments: a segment with count' < R, or one past the tile budget,
 * reports phases = R, phase = 0, per_phase = 0, metric all 0, n_hits =
 * n_written = 0, tail_window = -1, tail_errors = 0.
 *
 * Tile budget: the rule of "segmented acquisition" (B = ceil(Wmax /
 * DEMOD_ACQUIRE_TILE) + S tiles; a call's budget is the largest B its
 * work_bytes hold; segment s is scanned when the tiles of segments 0 .. s
 * together are within it).
 *
 * metric, phases, phase and per_phase of results[s] are byte-identical to the
 * same fields of demod_acquire_segments_async for the same tables. Every
 * output byte of a segment depends on its own contents and (count', R) alone:
 * not on first[s], the slot s, S, the grid or the neighbours. No
 * floating-point atomics, no atomic decides a position.
 */

/* Bytes of d_work for up to max_segments segments of a batch of up to
 * max_windows windows; monotone in both. With S = max_segments, B =
 * ceil(max_windows / DEMOD_ACQUIRE_TILE) + S tiles and R phases: the header of
 * the segmented acquisition, 20 S + 4 rounded up to 8, then per tile one
 * 8-byte partial and one 8-byte tail word per phase (16 B R), one 4-byte hit
 * count per phase (4 B R, rounded up to 8) and one 4-byte prefix (4 B, rounded
 * up to 8). 0 when the configuration is invalid (as
 * demod_frames_workspace_size), max_segments is 0 or above DEMOD_MAX_SEGMENTS,
 * or max_windows >= 2^31. No device needed. */
size_t demod_frames_segments_workspace_size(const demod_cfg_t *cfg, size_t max_segments,
                                            size_t max_windows);

/*
 * Enqueued on `stream`: five launches whatever n_segments and the hit counts
 * are (plan, scan, finalise, emit, gather; four when d_payload and d_packed
 * are both NULL or N == 0; three when max_frames == 0, which counts only).
 * Nothing is allocated or synchronised and the handle holds no state of the
 * call; d_work may hold anything on entry (every word a launch reads is
 * stored by an earlier launch of the same call; no atomics on d_work), so the
 * call can be captured behind demod_batch_async and replayed after the tables
 * are rewritten in place. d_hits is [n_segments][max_frames], d_payload
 * [n_segments][max_frames][N], d_packed [n_segments][max_frames][B] (either
 * may be NULL), d_results [n_segments]. Returns DEMOD_OK once enqueued;
 * DEMOD_BAD_ARG, before any launch, for what demod_frames_async refuses except
 * n_windows < R (a per-segment outcome here), n_segments == 0 or >
 * DEMOD_MAX_SEGMENTS, a NULL d_first or d_count, n_segments * max_frames >=
 * 2^31, work_bytes below demod_frames_segments_workspace_size(cfg, n_segments,
 * n_windows), or a misaligned d_hits, d_results, d_work, d_first (8 bytes) or
 * d_count (4 bytes).
 */
int demod_frames_segments_async(demod_t *st, const uint8_t *d_symbols, const float *d_mags,
                                size_t n_windows, const uint64_t *d_first, const uint32_t *d_count,
                                size_t n_segments, const uint8_t *sync, size_t sync_len,
                                uint32_t max_errors, size_t frame_symbols, demod_frame_hit_t *d_hits,
                                uint8_t *d_payload, uint8_t *d_packed, size_t max_frames,
                                demod_frames_result_t *d_results, void *d_work, size_t work_bytes,
                                void *stream);

/*
 * The handle's detector over the n_windows sliding windows of pcm (a host or
 * device pointer, as demod_acquire), then the segmented frame scan of its
 * outputs. first, count, hits ([n_segments][max_frames]), payload
 * ([n_segments][max_frames][N]) and packed ([n_segments][max_frames][B];
 * either may be NULL) and results are HOST memory; rows past a segment's
 * n_written are left alone. The tables are checked here, as
 * demod_acquire_segments checks them: a segment that leaves the batch or
 * holds fewer than R windows is refused with DEMOD_BAD_ARG before the
 * detector runs. The device keeps min(max_frames, longest / R + 1) rows per
 * segment. Synchronous; handle-owned buffers grow on first use. Returns the
 * sum of n_written or a negative code.
 */
int demod_frames_segments(demod_t *st, const int16_t *pcm, size_t n_windows, const uint64_t *first,
                          const uint32_t *count, size_t n_segments, const uint8_t *sync,
                          size_t sync_len, uint32_t max_errors, size_t frame_symbols,
                          demod_frame_hit_t *hits, uint8_t *payload, uint8_t *packed,
                          size_t max_frames, demod_frames_result_t *results);

/* ---- checked frames: length, CRC and overlap after a frame scan --------- */
/*
 * The frame scans above list every sync-word hit with a fixed-length row, false
 * hits and hits inside other frames included. This stage reads the rows they
 * wrote, on the device, and keeps the frames that check out. The frame is
 * defined on the packed row (B = ceil(N bits / 8) bytes, MSB first, as
 * demod_pack_symbols), with h = len_bytes in {1, 2} and c = 2 or 4 by CRC kind:
 *
 *   byte 0 .. h-1          len, big-endian
 *   byte h .. h+len-1      data
 *   byte h+len .. +c-1     CRC, big-endian, over bytes 0 .. h+len-1 (the length
 *                          field included)
 *   the rest of the row    ignored
 *
 *   max_len = B - h - c (a call with B < h + c is refused). A frame occupies
 *   L + S symbols: the word, then S = ceil((h + len + c) 8 / bits).
 *
 * Both CRC kinds are non-reflected with xorout 0:
 *
 *   DEMOD_CRC16_CCITT_FALSE  width 16, poly 0x1021, init 0xFFFF
 *                            (CRC of "123456789": 0x29B1)
 *   DEMOD_CRC32_MPEG2        width 32, poly 0x04C11DB7, init 0xFFFFFFFF
 *                            (CRC of "123456789": 0x0376E6E7)
 *
 * Groups and rows: group g < n_groups owns rows g max_frames + i, i < nw_g =
 * min(d_results[g].n_written, max_frames): what demod_frames_async (n_groups =
 * 1) or demod_frames_segments_async (n_groups = S) wrote for that batch or
 * segment, in ascending window order. The counts are read on the device and
 * clamped there; no content of d_results, d_hits or d_packed makes a kernel
 * read outside the rows or write outside the outputs. For each row i < nw_g:
 *
 *   length   the header value.
 *   status   DEMOD_CHECK_BAD_LENGTH when length > max_len (nothing past the
 *            header is read; crc is reported as 0); else crc = the CRC computed
 *            over bytes 0 .. h+len-1, and DEMOD_CHECK_BAD_CRC when the stored
 *            one differs, DEMOD_CHECK_OK otherwise.
 *   covered  with end_j = window_j + (L + S_j) R (64-bit, wrapping): 1 when
 *            row i is OK and some OK row j < i of the group has end_j >
 *            window_i, else 0. An exclusive prefix maximum over the OK rows:
 *            parallel and the same on every run. It is NOT the serial greedy
 *            hold-off (which lets a frame covered only by a covered frame
 *            through): the prefix maximum drops a superset of what greedy
 *            drops, and the two differ only when frames that pass their CRC
 *            overlap each other.
 *   kept     OK and not covered. d_kept[g max_frames + r] is the row index i
 *            of the group's r-th kept row, ascending; d_body[(g max_frames +
 *            r) max_len + b] is data byte b of that row, b < length (d_body
 *            may be NULL).
 *
 * d_summary[g] = {nw_g, rows OK, rows kept, 0}. Written: every byte of d_check
 * rows i < nw_g and of d_summary[0 .. n_groups); kept entries r < n_kept; body
 * bytes b < length of body rows r < n_kept. Nothing else.
 */
#define DEMOD_CRC16_CCITT_FALSE 1
#define DEMOD_CRC32_MPEG2       2

#define DEMOD_CHECK_OK          0
#define DEMOD_CHECK_BAD_LENGTH  1   /* len > max_len; crc reported as 0 */
#define DEMOD_CHECK_BAD_CRC     2

typedef struct demod_frame_check {
    uint32_t length, crc /* computed */, status, covered;
} demod_frame_check_t;

typedef struct demod_frames_check_result {
    uint64_t n_checked, n_valid, n_kept, reserved;
} demod_frames_check_result_t;

/* The CRC of data[0 .. len) by kind (0 for an unknown kind). No device needed. */
uint32_t demod_crc(int crc, const uint8_t *data, size_t len);

/* Bytes of a checked frame of len data bytes, h + len + c; DEMOD_BAD_ARG for a
 * bad kind or len_bytes, DEMOD_FRAME_TOO_LARGE for len above 256^h - 1 or
 * DEMOD_MAX_FRAME_PAYLOAD. */
long long demod_checked_frame_size(size_t len, int len_bytes, int crc);

/* The transmit side: len || data || CRC into out[0 .. cap); demod_unpack_symbols
 * turns the bytes into symbols (with a 0 byte behind them where bits does not
 * divide 8 (h + len + c): the last symbol's missing bits). Returns the bytes written, what
 * demod_checked_frame_size refuses, or DEMOD_BUFFER_TOO_SMALL. */
int demod_checked_frame_encode(const uint8_t *data, size_t len, int len_bytes, int crc,
                               uint8_t *out, size_t cap);

/*
 * Enqueued on `stream`: three launches whatever the counts are (check, select,
 * body; two when d_body is NULL or max_len == 0). No workspace; nothing is
 * allocated or synchronised and the handle keeps no state of the call, so it
 * can be captured behind demod_frames[_segments]_async and replayed. No atomic
 * decides a position; every output byte is a function of the inputs alone. R
 * and bits come from the handle's configuration; sync_len and frame_symbols are
 * the frame scan's. d_hits, d_packed and d_results are the frame scan's outputs
 * ([n_groups][max_frames] rows, [n_groups] results); d_check and d_kept are
 * [n_groups][max_frames], d_body [n_groups][max_frames][max_len], d_summary
 * [n_groups]. Returns DEMOD_OK once enqueued; DEMOD_BAD_ARG, before any launch,
 * for a NULL handle or pointer (d_body excepted), a misaligned d_hits,
 * d_results or d_summary (8 bytes), d_check or d_kept (4 bytes), n_groups == 0
 * or above DEMOD_MAX_SEGMENTS, max_frames == 0, n_groups * max_frames >= 2^31,
 * sync_len outside 1 .. DEMOD_MAX_SYNC, a bad len_bytes or crc, n % hop != 0 or
 * R > DEMOD_MAX_PHASES, B < h + c, or max_len > DEMOD_MAX_FRAME_PAYLOAD.
 */
int demod_frames_check_async(demod_t *st, const demod_frame_hit_t *d_hits, const uint8_t *d_packed,
                             const demod_frames_result_t *d_results, size_t n_groups,
                             size_t max_frames, size_t sync_len, size_t frame_symbols, int len_bytes,
                             int crc, demod_frame_check_t *d_check, uint32_t *d_kept, uint8_t *d_body,
                             demod_frames_check_result_t *d_summary, void *stream);

/*
 * The handle's detector over the n_windows sliding windows of pcm (a host or
 * device pointer, as demod_acquire), the frame scan of its outputs and the
 * check of the scan's rows. Only the kept frames come back: hits[r], lengths[r]
 * and body[r max_len .. r max_len + lengths[r]) for r < n_kept (body may be
 * NULL; bytes past a frame's length are left alone), HOST memory of max_frames
 * rows, with *result the scan's and *summary the check's. result->n_hits >
 * result->n_written says that max_frames cut the scan. Synchronous;
 * handle-owned buffers grow on first use. Returns n_kept or a negative code
 * (DEMOD_BAD_ARG for what demod_frames and demod_frames_check_async refuse,
 * before the detector runs).
 */
int demod_frames_checked(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                         size_t sync_len, uint32_t max_errors, size_t frame_symbols, int len_bytes,
                         int crc, demod_frame_hit_t *hits, uint32_t *lengths, uint8_t *body,
                         size_t max_frames, demod_frames_result_t *result,
                         demod_frames_check_result_t *summary);

/* ---- coded frames: soft-decision Viterbi decode of a frame scan's rows --- */
/*
 * The check above drops a frame for one wrongly decided payload symbol. Here
 * the frame is convolutionally coded and a stage between the scan and the
 * check decodes each row from the per-tone powers P[W][K] the detector left
 * beside the symbols; the hard symbols are not read:
 *
 *   demod_frames[_segments]_async   (hits and results; d_packed, d_payload NULL)
 *     -> demod_frames_decode_async       soft values from d_mags, Viterbi, rows
 *     -> demod_frames_check_coded_async  the check's launches over those rows
 *
 * All arithmetic is integer apart from one double expression per soft value;
 * every output byte is a function of the inputs alone, the same on the device
 * and in demod_coded_frame_decode. K must be a power of two (K = 2^bits; a
 * coded bit would otherwise ask for a tone that does not exist): every entry
 * that takes K refuses another with DEMOD_BAD_ARG.
 *
 * `fec` is a bit field. The low nibble names the code, DEMOD_FEC_CONV_K7; at
 * most one of DEMOD_FEC_RATE_2_3 and DEMOD_FEC_RATE_3_4 punctures it, and
 * DEMOD_FEC_INTERLEAVE spreads its bits over 16 x 16 blocks ("punctured and
 * interleaved" below). Six values are valid, 1 | {0, 0x10, 0x20} | {0, 0x40};
 * every entry that takes `fec` refuses another with DEMOD_BAD_ARG (0, no
 * code, where it is accepted). DEMOD_FEC_CONV_K7 alone is rate 1/2 with the
 * coded bits on the air in order, and what follows describes it.
 *
 * The mother code: constraint length 7, rate 1/2,
 * generators 0171 and 0133 (octal). reg_-1 = 0, reg_t = ((reg_t-1 << 1) | u_t)
 * & 0x7F, v_2t = parity(reg_t & 0171), v_2t+1 = parity(reg_t & 0133); the state
 * after step t is reg_t & 63. The information bits u_t are the checked frame
 * len || data || CRC (n = h + len + c bytes, MSB first) and 0 for t >= 8 n,
 * for T(len) = max(8 n + 6, 8 h + DEMOD_FEC_DEPTH) steps: six tail bits, and
 * for short frames zero fill, so that the decoder's header look-ahead stays
 * inside the frame. A coded frame is 2 T bits, MSB first in ceil(2 T / 8)
 * bytes, pad bits 0; on the air it occupies L + Sc symbols, Sc = ceil(2 T /
 * bits).
 *
 * Soft values: symbol j of a row sits at window w_j = base_g + window_i + (L +
 * j) R, base_g = 0 without a segment table and min(d_first[g], n_windows) with
 * one. Soft value m = j bits + b (bit b of the symbol, MSB first): a0 = the
 * maximum of P[w_j][k] over the tones k < K whose bit b is 0, a1 over those
 * whose bit b is 1, each maximum started from the lowest such k and replaced in
 * ascending k by a strictly greater value alone; in double d = a0 - a1, s =
 * |a0| + |a1|; q_m = (int) rint(127 d / s) (to nearest even) when s > 0 and s
 * is finite, else 0. |q| <= 127. window_i >= n_windows or w_j >= n_windows (no
 * wrap-around) gives q_m = 0, an erasure: no content of d_hits, d_first or
 * d_results moves a read outside d_mags. The value is normalised per symbol:
 * a faded symbol weighs as much as a loud one.
 *
 * The decoder, per row of C = N bits soft values: St = floor(C / 2) steps (an
 * odd C leaves its last value unused), Bd = (St - 6) / 8 decoded bytes,
 * max_len = Bd - h - c. Refused: St < 8 h + DEMOD_FEC_DEPTH, Bd < h + c,
 * max_len > DEMOD_MAX_FRAME_PAYLOAD.
 *
 *   forward  int32 metrics, M[0] = 0 and M[s != 0] = -2^28. At step t state s
 *            has u = s & 1 and predecessors p0 = s >> 1, p1 = p0 | 32; the
 *            branch from p has register (p << 1) | u, expected bits c0, c1 as
 *            the encoder gives them and metric bm = (c0 ? -q_2t : q_2t) + (c1 ?
 *            -q_2t+1 : q_2t+1); M'[s] = max(M[p0] + bm0, M[p1] + bm1) and the
 *            decision d_t[s] = 1 only when the p1 sum is strictly greater.
 *   header   at t0 = 8 h + DEMOD_FEC_DEPTH the state of the greatest metric
 *            (ties: the lowest state) is traced back to step 0 (u_t = s & 1, s
 *            <- (s >> 1) | (d_t[s] << 5)); the first 8 h bits are len.
 *   len > max_len   status DEMOD_DECODE_BAD_LENGTH, length = len, metric = 0,
 *            steps = 0; the h header bytes of the row alone are written (the
 *            check then reports DEMOD_CHECK_BAD_LENGTH).
 *   else     traced back from state 0 at step T(len); bytes 0 .. n-1 of the row
 *            are written; status DEMOD_DECODE_OK, length = len, metric =
 *            M_T[0], steps = T.
 *
 * Row bytes at or past what is written, and rows i >= nw_g, are left alone.
 *
 * Punctured and interleaved. Both are one map between the trellis's coded-bit
 * index and the position on the air; T(len), the encoder, the tail and the
 * soft-value expression do not change. Mother bit m = 2 t + v (v = 0:
 * generator 0171, v = 1: 0133). Puncturing is by step phase: rate 2/3 (period
 * 2) keeps v0 v1 at phase 0 and v1 at phase 1; rate 3/4 (period 3) keeps v0 v1
 * at phase 0, v0 at phase 1 and v1 at phase 2 (free distance 6 and 5; the
 * mother code's is 10). T steps keep Nt(T) bits: 2 T, 3 floor(T / 2) + 2 (T
 * mod 2) or 4 floor(T / 3) + {0, 2, 3}[T mod 3]. A kept bit's code index is i
 * = Nt(t) + its rank among step t's kept bits. With DEMOD_FEC_INTERLEAVE, i =
 * r 16 + c of each block of DEMOD_FEC_IL_ROWS x DEMOD_FEC_IL_COLS code bits
 * goes to air position a = c 16 + r (the two nibbles of the low byte swapped:
 * an involution, the same function at both ends); otherwise a = i. A frame
 * is Na(len) = Nt(T(len)) air bits, rounded up to a multiple of 256 with the
 * flag; positions no kept bit maps to carry 0 and are never read; Sc = ceil(Na
 * / bits). A row of C = N bits soft values uses Cu = C (C & ~255 with the
 * flag); St is the greatest T with Nt(T) <= Cu; Bd, max_len and the refusals
 * follow from St as above (an interleaved row shorter than one block is
 * refused). Trellis soft value q_m is the soft value at air position a(m), or
 * 0 where m is punctured, which is not read.
 */
#define DEMOD_FEC_CONV_K7       1      /* low nibble: the code. Alone: rate 1/2, in order */
#define DEMOD_FEC_RATE_2_3      0x10
#define DEMOD_FEC_RATE_3_4      0x20   /* both rate flags together: refused */
#define DEMOD_FEC_INTERLEAVE    0x40
#define DEMOD_FEC_IL_ROWS       16
#define DEMOD_FEC_IL_COLS       16     /* block = 256 air bits */
#define DEMOD_FEC_DEPTH         64

#define DEMOD_DECODE_OK         0
#define DEMOD_DECODE_BAD_LENGTH 1   /* len > max_len; metric and steps 0 */

typedef struct demod_frame_decode {
    uint32_t length;
    int32_t metric;
    uint32_t status, steps;
} demod_frame_decode_t;

/* T(len), or what demod_checked_frame_size refuses. No device needed. */
long long demod_coded_frame_steps(size_t len, int len_bytes, int crc);

/* Sc = ceil(2 T(len) / bits); DEMOD_BAD_ARG also for bits outside 1 .. 4. */
long long demod_coded_frame_symbols(size_t len, int len_bytes, int crc, int bits);

/* The transmit side: the coded bits of len || data || CRC into out[0 .. cap),
 * ceil(2 T / 8) bytes that demod_unpack_symbols turns into Sc symbols. Returns
 * the bytes written, what demod_checked_frame_encode refuses, or
 * DEMOD_BUFFER_TOO_SMALL. */
int demod_coded_frame_encode(const uint8_t *data, size_t len, int len_bytes, int crc, uint8_t *out,
                             size_t cap);

/* Bd of rows of frame_symbols symbols; DEMOD_BAD_ARG for bits outside 1 .. 4,
 * a bad len_bytes, frame_symbols >= 2^31 or St < 8 h + DEMOD_FEC_DEPTH. */
long long demod_coded_row_bytes(size_t frame_symbols, int bits, int len_bytes);

/* The soft values of one window: soft[b], b < bits, from powers[0 .. k).
 * Returns bits, or DEMOD_BAD_ARG for a NULL pointer or k not 2, 4, 8 or 16. */
int demod_soft_bits(const float *powers, uint32_t k, int8_t *soft);

/* The decoder above on a host array of n_soft = C soft values: the reference of
 * demod_frames_decode_async. row[0 .. cap) must hold Bd bytes
 * (DEMOD_BUFFER_TOO_SMALL otherwise). Returns the row bytes written (h or n),
 * DEMOD_BAD_ARG for a NULL pointer, a bad len_bytes or crc or a refused row
 * shape, or DEMOD_ALLOC_FAIL. */
int demod_coded_frame_decode(const int8_t *soft, size_t n_soft, int len_bytes, int crc, uint8_t *row,
                             size_t cap, demod_frame_decode_t *decode);

/* The same five with a mode ("punctured and interleaved"); the functions
 * above equal them at fec == DEMOD_FEC_CONV_K7. Each refuses an invalid fec
 * with DEMOD_BAD_ARG.
 *   air_index      the air position of mother bit m < 2^31, or -1 when it is
 *                  punctured (or fec is invalid)
 *   frame_symbols  Sc of the mode
 *   frame_encode   the frame in air order, ceil(Na / 8) bytes, pad bits 0
 *   row_bytes      Bd of the mode's St
 *   frame_decode   soft[0 .. n_soft) in air order, n_soft = C: the reference of
 *                  demod_frames_decode_async in every mode, bit for bit */
long long demod_fec_air_index(int fec, size_t m);
long long demod_fec_frame_symbols(size_t len, int len_bytes, int crc, int bits, int fec);
int demod_fec_frame_encode(const uint8_t *data, size_t len, int len_bytes, int crc, int fec, uint8_t *out,
                           size_t cap);
long long demod_fec_row_bytes(size_t frame_symbols, int bits, int len_bytes, int fec);
int demod_fec_frame_decode(const int8_t *soft, size_t n_soft, int len_bytes, int crc, int fec, uint8_t *row,
                           size_t cap, demod_frame_decode_t *decode);

/* Bytes of d_work: the launch's waves (min(max_frames, max(16384 / n_groups,
 * 1)) per group, as the check caps them) x St x 8, the survivor words of each
 * wave's current row. 0 when the configuration is invalid, K is not a power of
 * two, n_groups is 0 or above DEMOD_MAX_SEGMENTS, max_frames is 0, n_groups *
 * max_frames >= 2^31, or frame_symbols is 0 or >= 2^31. No device needed. */
size_t demod_frames_decode_workspace_size(const demod_cfg_t *cfg, size_t n_groups, size_t max_frames,
                                          size_t frame_symbols);

/* The same with the mode's St, which a punctured row raises to as much as 3/4
 * of C: what demod_frames_decode_async asks of work_bytes. Equals the function
 * above at fec == DEMOD_FEC_CONV_K7; 0 also for an invalid fec. */
size_t demod_fec_decode_workspace_size(const demod_cfg_t *cfg, size_t n_groups, size_t max_frames,
                                       size_t frame_symbols, int fec);

/*
 * Enqueued on `stream`: one launch whatever the counts are. Nothing is
 * allocated or synchronised, no atomics, and the handle keeps no state of the
 * call; d_work may hold anything on entry (every word read is written first by
 * the same call), so the call can be captured behind either scan and replayed
 * after the powers and the tables were rewritten in place. Groups and rows as
 * "checked frames": group g owns rows g max_frames + i, i < nw_g. d_hits and
 * d_results are the scan's; d_mags [n_windows][K] the detector's; d_first NULL
 * (every base 0) or the segmented scan's table [n_groups]; d_rows is
 * [n_groups][max_frames][Bd], d_decode [n_groups][max_frames]. Returns DEMOD_OK
 * once enqueued; DEMOD_BAD_ARG, before any launch, for what
 * demod_frames_check_async refuses about its own arguments and: K not a power
 * of two, the refused row shapes above, a fec that is not one of the six modes
 * (each with or without a parity flag of "Reed-Solomon outer code"), a NULL
 * d_mags, d_rows, d_decode or d_work, a misaligned d_decode (4 bytes), d_work
 * or d_first (8 bytes), work_bytes below demod_fec_decode_workspace_size,
 * n_windows >= 2^31, (sync_len + frame_symbols) R >= 2^31.
 */
int demod_frames_decode_async(demod_t *st, const demod_frame_hit_t *d_hits, const float *d_mags,
                              size_t n_windows, const uint64_t *d_first,
                              const demod_frames_result_t *d_results, size_t n_groups,
                              size_t max_frames, size_t sync_len, size_t frame_symbols, int len_bytes,
                              int crc, int fec, uint8_t *d_rows, demod_frame_decode_t *d_decode,
                              void *d_work, size_t work_bytes, void *stream);

/*
 * demod_frames_check_async over decoded rows: the same launches and outputs
 * with the row width Bd and, for `covered`, the coded span S = ceil(2 T(len) /
 * bits); max_len = Bd - h - c in the six coded modes. Refuses what
 * demod_frames_check_async and demod_frames_decode_async refuse about the same
 * arguments. Takes the 20 modes of "Reed-Solomon outer code": with a parity
 * flag max_len is the greatest len with n'(len) <= the row width and the span
 * follows n'; with the low nibble 0 the rows are the scan's packed rows of B
 * bytes and the span is ceil(8 n' / bits).
 */
int demod_frames_check_coded_async(demod_t *st, const demod_frame_hit_t *d_hits, const uint8_t *d_rows,
                                   const demod_frames_result_t *d_results, size_t n_groups,
                                   size_t max_frames, size_t sync_len, size_t frame_symbols,
                                   int len_bytes, int crc, int fec, demod_frame_check_t *d_check,
                                   uint32_t *d_kept, uint8_t *d_body,
                                   demod_frames_check_result_t *d_summary, void *stream);

/*
 * demod_frames_checked for coded frames: detector, frame scan (no packed rows),
 * decode, coded check and the kept rows, on handle-owned buffers. Arguments,
 * outputs and return value as demod_frames_checked, with the mode's max_len:
 * Bd - h - c in the six coded modes. Takes the 20 modes of "Reed-Solomon outer
 * code": with a parity flag max_len is the greatest len with n'(len) <= the
 * row width and demod_frames_rs_async runs before the check; with the low
 * nibble 0 the scan writes packed rows (the row width is B) and nothing is
 * decoded.
 */
int demod_frames_coded(demod_t *st, const int16_t *pcm, size_t n_windows, const uint8_t *sync,
                       size_t sync_len, uint32_t max_errors, size_t frame_symbols, int len_bytes,
                       int crc, int fec, demod_frame_hit_t *hits, uint32_t *lengths, uint8_t *body,
                       size_t max_frames, demod_frames_result_t *result,
                       demod_frames_check_result_t *summary);

/* ---- Reed-Solomon outer code: a few wrong bytes, wherever they sit -------- */
/*
 * The CRC only detects. At fec == 0 one wrongly decided symbol loses the
 * frame; in a coded mode the frame is lost whenever the Viterbi decoder leaves
 * the correct path, and its errors then come as a short burst of wrong bytes.
 * A byte-oriented outer code corrects both. Two more flags of `fec` name it:
 *
 *   DEMOD_FEC_RS16  P = 16 parity bytes a codeword, t = 8 wrong bytes corrected
 *   DEMOD_FEC_RS32  P = 32, t = 16                  (both together: refused)
 *
 * Each of the six coded modes takes none or one of them, and each flag stands
 * alone (low nibble 0: no convolutional code): 20 non-zero values in all.
 *
 * The field is GF(2^8) with the reduction polynomial 0x11D and alpha = 2; the
 * generator is g(x) = prod_{i < P} (x - alpha^i). A codeword of the message
 * m[0 .. k) is systematic: m[0] is the highest coefficient, the parity is the
 * remainder of m(x) x^P by g, highest degree first, and the codeword is m ||
 * parity, shortened (the missing leading symbols are 0 and are never sent).
 *
 * The protected frame. With F = len || data || CRC, the n = h + len + c bytes
 * of "checked frames", and k_max = 255 - P: D = ceil(n / k_max) codewords,
 * byte-interleaved. Codeword j < D has the message bytes F[j], F[j + D], ..
 * (k_j = ceil((n - j) / D) of them); the frame is F followed by D P parity
 * bytes, parity byte i D + j being byte i of codeword j's parity. n'(len) = n +
 * D P, which increases strictly with len. With the low nibble 0 the n' bytes go
 * on the air as a plain frame does, S = ceil(8 n' / bits) symbols; with
 * DEMOD_FEC_CONV_K7 they are the information bits of the unchanged trellis,
 * T(len) = max(8 n' + 6, 8 h + DEMOD_FEC_DEPTH).
 *
 * Rows of W bytes (B, or Bd in a coded mode) hold max_len = the greatest len
 * with n'(len) <= W; W < n'(0) and max_len > DEMOD_MAX_FRAME_PAYLOAD are
 * refused.
 *
 * The length header is read as it is: from the row, or by the Viterbi header
 * look-ahead. It is covered by codeword 0 (and codeword 1 when h = 2 and D >=
 * 2), so a wrong header is detected (the codewords it lays out do not decode,
 * or the CRC fails), not repaired: a frame whose header bytes are wrong is
 * lost.
 *
 * The decoder is defined by its result. For each codeword, with the received
 * word r of k_j + P symbols: if a codeword c of the shortened code has d(r, c)
 * <= t it is unique, r is replaced by c and e_j = d; otherwise the codeword's
 * bytes stay as they are and it counts as failed (a locator with a root outside
 * the k_j + P positions, or with fewer roots than its degree, is a failure).
 * The record of a row:
 *
 *   status     DEMOD_RS_OK every codeword decoded; DEMOD_RS_BAD_LENGTH len >
 *              max_len (nothing past the header is read, the other fields 0);
 *              DEMOD_RS_FAILED at least one codeword failed (the others are
 *              still corrected)
 *   codewords  D;  corrected  sum of e_j;  failed  the codewords that failed
 *
 * The CRC stays the arbiter of a frame: the check does not read this record.
 *
 * Erasure decoding. The detector knows which bytes to doubt: in a dropout or a
 * fade the tones of a window are indistinguishable, the hard symbol is a coin
 * toss, and the soft value q_m of "coded frames" is near 0. A decoder that is
 * told where the doubtful bytes are corrects twice as many: with f flagged
 * bytes in a codeword it corrects e further wrong ones as long as 2 e + f <= P.
 *
 * The erasure mask is one bit per row byte. Row r = g max_frames + i has Wm =
 * ceil(row_bytes / 64) uint64_t words; byte b is bit b & 63 of word b >> 6; the
 * mask is 8-byte aligned. Bits at b >= row_bytes are written as 0 by the
 * producer and ignored by the decoder. One wave's ballot over 64 consecutive
 * row bytes is one word of it.
 *
 * The decoder with a mask, again by its result. For codeword j let E be the
 * positions of the received word r whose row byte is flagged, f = |E|.
 *   f = 0 or f > P   exactly the rule above (errors only).
 *   1 <= f <= P      first attempt: if a codeword c of the shortened code has
 *                    2 |{x not in E : r_x != c_x}| + f <= P it is unique (two
 *                    such words would differ in at most e1 + e2 + f <= P
 *                    places); r is replaced by c and e_j is the number of bytes
 *                    that changed, erased ones included (a flagged byte that
 *                    was right costs nothing but its share of f). Otherwise the
 *                    fallback: the rule above on the same word; if that fails
 *                    too the bytes stay and the codeword counts as failed.
 * A word with zero syndromes is its own codeword under every branch and is
 * left as it is whatever the mask holds; it counts in neither `used` nor
 * `fallback`. The length header is read as it is, as above, and the CRC stays
 * the arbiter: with f = P any word "decodes". Beside demod_frame_rs_t (its
 * fields as above) a row has a second record, demod_frame_erase_t:
 *
 *   erased    the flagged bytes among the frame's n' bytes
 *   used      the codewords accepted by the first attempt
 *   fallback  the codewords with f >= 1 and non-zero syndromes that were
 *             accepted or failed under the errors-only rule: f > P, or the
 *             first attempt found nothing
 *   reserved  0
 *
 * all 0 with DEMOD_RS_BAD_LENGTH.
 *
 * The level. DEMOD_FEC_ERASE(level), level 1 .. 127, in `fec` asks the one-shot
 * call and the receiver to flag byte b of a plain row where the least |q_m|
 * over its eight air bits m = 8 b .. 8 b + 7 is below the level (q_m = 0 for m
 * >= N bits), and to run the decoder with that mask. It is accepted only
 * together with a parity flag and low nibble 0 (the Viterbi decoder's own
 * reliability is not passed on), and only by demod_frames_coded,
 * demod_rx_create and demod_rx_sizes; every other entry refuses
 * it as it refuses any unknown bit. The frame on the air is the same: a
 * transmitter is created with the mode without the field.
 *
 * Not here: passing the Viterbi decoder's reliability to the outer code,
 * retries at several levels, protecting the length header, the multi-GPU
 * group, fskrx options.
 *
 * Every entry that takes `fec` takes the 20 modes where the frame alone is
 * concerned (the check, the one-shot call, the receiver, the transmitter, the
 * demod_rs_* codec); the trellis's own functions (demod_fec_*,
 * demod_frames_decode_async) refuse a mode without the convolutional code and
 * size the frame by n', and demod_fec_frame_decode is the Viterbi part alone,
 * writing n' bytes.
 */
#define DEMOD_FEC_RS16          0x100
#define DEMOD_FEC_RS32          0x200  /* both parity flags together: refused */

#define DEMOD_RS_OK             0
#define DEMOD_RS_BAD_LENGTH     1   /* len > max_len; the other fields 0 */
#define DEMOD_RS_FAILED         2   /* at least one codeword failed */

typedef struct demod_frame_rs {
    uint32_t status, codewords, corrected, failed;
} demod_frame_rs_t;

#define DEMOD_FEC_ERASE(level)  (((level) & 0x7F) << 16)   /* only with a parity flag and low nibble 0 */

typedef struct demod_frame_erase {
    uint32_t erased, used, fallback, reserved;
} demod_frame_erase_t;

/* The host codec; no device needed. `fec` is any of the 20 modes (without a
 * parity flag n' = n and there is nothing to decode); another value is refused
 * with DEMOD_BAD_ARG.
 *   generator     g of 1 <= parity_bytes <= 32 roots into g[0 .. parity_bytes],
 *                 highest coefficient first; returns parity_bytes + 1
 *   encode        the parity of one codeword's message msg[0 .. k), k +
 *                 parity_bytes <= 255; returns parity_bytes
 *   frame_size    n'(len), or what demod_checked_frame_size refuses
 *   max_len       of rows of row_bytes bytes; DEMOD_BAD_ARG when none fits
 *   frame_encode  the n' bytes into out[0 .. cap); returns n', what
 *                 demod_checked_frame_encode refuses or DEMOD_BUFFER_TOO_SMALL
 *   frame_decode  the decoder above on row[0 .. cap), in place: the reference
 *                 of demod_frames_rs_async, bit for bit. cap is the row width
 *                 W that decides max_len. Returns the bytes it covered (n', or h
 *                 with DEMOD_RS_BAD_LENGTH), or DEMOD_BAD_ARG for a NULL
 *                 pointer, a bad len_bytes, crc or fec or a refused row width. */
int demod_rs_generator(int parity_bytes, uint8_t *g);
int demod_rs_encode(const uint8_t *msg, size_t k, int parity_bytes, uint8_t *parity);
long long demod_rs_frame_size(size_t len, int len_bytes, int crc, int fec);
long long demod_rs_max_len(size_t row_bytes, int len_bytes, int crc, int fec);
int demod_rs_frame_encode(const uint8_t *data, size_t len, int len_bytes, int crc, int fec, uint8_t *out,
                          size_t cap);
int demod_rs_frame_decode(uint8_t *row, size_t cap, int len_bytes, int crc, int fec, demod_frame_rs_t *out);

/* frame_decode with a mask ("erasure decoding"): the reference of
 * demod_frames_rs_erasures_async, bit for bit. erase is the row's Wm words of
 * cap bytes, or NULL for no flags; the row, *out and the return value are then
 * demod_rs_frame_decode's and *erec is 0. Takes the modes that carry a parity
 * flag (without a level). DEMOD_BAD_ARG also for a NULL erec or a misaligned
 * erase (8 bytes). */
int demod_rs_frame_decode_erasures(uint8_t *row, size_t cap, int len_bytes, int crc, int fec,
                                   const uint64_t *erase, demod_frame_rs_t *out, demod_frame_erase_t *erec);

/* The mask of one plain row from its soft values in air order (demod_soft_bits
 * of each window, n_soft = N bits of them): byte b < row_bytes is flagged iff
 * the least |soft[m]| over m = 8 b .. 8 b + 7 is below level, soft[m] = 0 for m
 * >= n_soft. Writes the Wm words of row_bytes bytes and returns Wm; with
 * demod_soft_bits the reference of demod_frames_erasures_async.
 * DEMOD_BAD_ARG for a NULL pointer, a misaligned erase (8 bytes), a level
 * outside 1 .. 127, row_bytes 0 or >= 2^31. */
int demod_soft_erasures(const int8_t *soft, size_t n_soft, int level, uint64_t *erase, size_t row_bytes);

/*
 * The device stage, between the scan (low nibble 0: over its d_packed) or
 * demod_frames_decode_async (a coded mode: over its d_rows) and
 * demod_frames_check_coded_async. Enqueued on `stream`: one launch whatever the
 * counts are. No workspace, no atomics, no floating point; nothing is allocated
 * or synchronised and the handle keeps no state of the call, so it can be
 * captured behind the scan and replayed. Groups and rows as "checked frames";
 * the counts are read and clamped on the device, and no content of a row or a
 * result moves a read or a write outside the rows. It corrects the rows in
 * place. Written: bytes among the first n'(len) of rows i < nw_g that a decoded
 * codeword changes; every byte of their d_rs records ([n_groups][max_frames]);
 * nothing else. Returns DEMOD_OK once enqueued; DEMOD_BAD_ARG, before the
 * launch, for what demod_frames_check_coded_async refuses about the same
 * arguments, a fec without a parity flag, a NULL d_rs or one misaligned (4
 * bytes).
 */
int demod_frames_rs_async(demod_t *st, uint8_t *d_rows, const demod_frames_result_t *d_results,
                          size_t n_groups, size_t max_frames, size_t frame_symbols, int len_bytes, int crc,
                          int fec, demod_frame_rs_t *d_rs, void *stream);

/*
 * The mask's producer, behind either scan over plain (uncoded) rows. Enqueued
 * on `stream`: one launch, no workspace, no atomics, nothing allocated or
 * synchronised, capturable behind the scan. One thread per row byte; air bit m
 * of a row is the soft value q_m of "coded frames" with a = m: the same window
 * arithmetic (d_first NULL or the segmented scan's table), maxima and double
 * expression, no wrap-around; a hit's window, or a symbol's, at or past
 * n_windows gives 0 and is not read, m >= N bits gives 0. d_erase is
 * [n_groups][max_frames][Wm] words, Wm of B = ceil(N bits / 8) bytes; every
 * word of every row i < nw_g is written, no other row is touched. The counts
 * are read and clamped on the device. Returns DEMOD_OK once enqueued;
 * DEMOD_BAD_ARG, before the launch, for a NULL pointer (d_first may be), a
 * misaligned d_hits, d_results, d_first or d_erase (8 bytes), K not 2, 4, 8 or
 * 16, a level outside 1 .. 127, what demod_frames_check_async refuses about
 * the configuration, the groups and rows and sync_len, frame_symbols 0 or B
 * above 4710 (the widest row any mode with a parity flag takes); also
 * n_windows >= 2^31 and (sync_len + frame_symbols) R >= 2^31.
 */
int demod_frames_erasures_async(demod_t *st, const demod_frame_hit_t *d_hits, const float *d_mags,
                                size_t n_windows, const uint64_t *d_first,
                                const demod_frames_result_t *d_results, size_t n_groups, size_t max_frames,
                                size_t sync_len, size_t frame_symbols, int level, uint64_t *d_erase,
                                void *stream);

/*
 * demod_frames_rs_async with a mask: the decoder of "erasure decoding" on the
 * rows, in place. d_erase is [n_groups][max_frames][Wm] words, Wm of the row
 * width (B, or Bd in a coded mode: a caller with a reliability of their own can
 * run it behind the Viterbi decode), d_erec [n_groups][max_frames]. Launch,
 * rows, counts and what is written as demod_frames_rs_async, and every byte of
 * the d_erec records of rows i < nw_g. An all-zero mask gives exactly
 * demod_frames_rs_async's rows and records. Takes the modes with a parity flag
 * (without a level); refuses what demod_frames_rs_async refuses, a NULL d_erase
 * or d_erec, a misaligned d_erase (8 bytes) or d_erec (4 bytes).
 */
int demod_frames_rs_erasures_async(demod_t *st, uint8_t *d_rows, const uint64_t *d_erase,
                                   const demod_frames_result_t *d_results, size_t n_groups, size_t max_frames,
                                   size_t frame_symbols, int len_bytes, int crc, int fec,
                                   demod_frame_rs_t *d_rs, demod_frame_erase_t *d_erec, void *stream);

/* ---- many streams, one launch (config 5 as a service) ----------------- */
/*
 * n_streams independent streams that share one configuration, each behaving
 * exactly like its own demod_t from that cfg (its own carry buffer and
 * lead-in). The reference runs one decoder per device (playback.cpp:157-165);
 * a receiver of many streams would otherwise make one demodulate() call --
 * one H2D copy, one kernel launch, one D2H copy -- per stream per packet.
 * demod_streams_push takes one packet per stream and demodulates every
 * complete window of every stream in ONE batch: one copy in, one detector
 * launch, one copy out (the streams' runs laid end to end on hop
 * boundaries; windows that would straddle two runs are computed and
 * dropped).
 */
typedef struct demod_streams demod_streams_t;

/* NULL on failure, *error set. n_streams >= 1. */
demod_streams_t *demod_streams_create(const demod_cfg_t *cfg, size_t n_streams, int *error);
void demod_streams_destroy(demod_streams_t *ms);

/* demod_reset for one stream (drop its carry, re-arm cfg.lead_in). */
int demod_streams_reset(demod_streams_t *ms, size_t stream);

/* Mono samples stream `stream` carries between pushes. */
int demod_streams_pending(const demod_streams_t *ms, size_t stream);

/* Upper bound on the symbols the next push with these packet sizes emits. */
long long demod_streams_max_symbols(const demod_streams_t *ms, const size_t *n_frames);

/*
 * pcm[i]: host pointer to n_frames[i] frames of stream i (`channels`
 * interleaved int16, as for demodulate; NULL allowed when n_frames[i] == 0).
 * Symbols of stream 0, then stream 1, ... are written to symbols[0..];
 * counts[i] receives the number stream i emitted; mags (nullable, host)
 * receives k floats |X_k|^2 per symbol in the same order. Returns the total,
 * or a negative code; if cap is too small nothing is consumed and
 * DEMOD_BUFFER_TOO_SMALL is returned. Symbols and magnitudes equal what
 * per-stream demodulate() calls would return.
 */
int demod_streams_push(demod_streams_t *ms, const int16_t *const *pcm, const size_t *n_frames,
                       uint8_t *symbols, float *mags, size_t cap, uint32_t *counts);

/*
 * The packet front-end of many streams (SURVEY §8 f2's decoder-agnostic half):
 * one encoded packet per stream, each decoded by `decode` with its stream's
 * decoder state, then demodulated as by demod_streams_push (per-stream carry,
 * lead-in, one batch). demod_decode_fn has opus_decode's signature
 * (libopus/src/opus.h:462; opus_decode itself, cast, is one), as the
 * reference calls it per packet (playback.cpp:115-122): it writes at most
 * frame_size frames of `channels` interleaved int16 to pcm and returns the
 * frames decoded or a negative code. decoders[i] is stream i's state (used by
 * one thread at a time: streams decode concurrently on the handle's staging
 * threads). lens[i] == 0: no packet for stream i this push (playback.cpp:105).
 * A decoder's negative code (the lowest stream's) is returned with nothing
 * pushed. Otherwise as demod_streams_push.
 */
typedef int (*demod_decode_fn)(void *decoder, const unsigned char *data, int32_t len, int16_t *pcm,
                               int frame_size, int decode_fec);
int demod_streams_push_packets(demod_streams_t *ms, demod_decode_fn decode, void *const *decoders,
                               const uint8_t *const *packets, const int32_t *lens, int frame_size,
                               uint8_t *symbols, float *mags, size_t cap, uint32_t *counts);

/* ---- receiver: frames of live streams, carried on the device ------------- */
/*
 * demod_streams_push ends at raw symbols, and the frame stages above work on
 * one finished batch: a frame that starts in one packet and ends in a later one
 * needs a carry. The receiver keeps that carry on the device, in the detector's
 * OUTPUT domain (1 + 4 K bytes a window instead of 2 hop bytes of samples), so
 * the detector sees no sample twice, and returns the checked (or decoded and
 * checked) frames of all streams as one dense list.
 *
 * Per stream the receiver holds a run X of detector outputs, sym[i] and
 * P[i][K] for i < fill; window i is the stream's window base + i, counted from
 * create or reset. With X it holds keep, hold and the counters dropped and
 * cut_hits; all are 0 initially. C = ring_windows; R, L, N, h, c, bits, the
 * span S and `complete` are as in the sections above. A push with `new` fresh
 * windows for the stream does, in this order:
 *
 *   1 advance  keep' = min(keep, fill); Y = X[keep' ..) followed by the new
 *              windows; base += keep'. If len(Y) > C the oldest d = len(Y) - C
 *              windows of Y go: base += d, dropped += d. X = Y, fill = len(Y).
 *   2 scan     X is scanned exactly as segment {first = slot, count = fill} of
 *              "segmented frame scan" (group = stream). fec == 0: packed rows,
 *              then "checked frames". A coded mode: no rows, then
 *              the decode and the coded check of "coded frames".
 *   3 collect  For the OK rows end_j = base + window_j + (L + S_j) R, S_j the
 *              span the check's `covered` uses (plain or coded). A kept row i
 *              is EMITTED when base + window_i >= hold, hold as the pushes
 *              before left it (kept rows ascend: the rows not emitted are a
 *              prefix). Then hold = max(hold, the largest end_j of this push,
 *              covered rows included); keep = max(0, t - (R - 1)), where t is
 *              tail_window when the result's tail_window >= 0, else fill - (L -
 *              1) R: every start, on any phase, whose word does not fit yet.
 *              The R - 1 windows below t hold the same word's start on the
 *              other phases, for a next push that chooses one of them;
 *              cut_hits += n_hits - n_written.
 *   4 output   the emitted rows of stream 0, then stream 1, ..., each in
 *              ascending window order; a row's data bytes at `body`, the
 *              exclusive prefix of `length` in that order.
 *
 * With no overflow (dropped == 0), no cut (cut_hits == 0) and the same absolute
 * phase (base + phase) mod R chosen at every push, the frames a stream emits
 * over all pushes are exactly the kept frames of demod_frames_checked (or
 * demod_frames_coded) on the whole recording, in the same order, whatever the
 * packet sizes: the R - 1 windows kept below t lie on other phases and add no
 * hit. The phase is decided per push over X alone, and two neighbouring phases
 * tie when a symbol boundary lies half-way between them: the choice then flips
 * from push to push. A frame whose word is a hit (max_errors or fewer errors)
 * on the phase of every push, from the one in which its word first fits to the
 * one in which its row is complete, is still received, once, at a window
 * within R - 1 of the one-shot's: each of those pushes leaves keep at or below
 * the word's start on any phase, and `hold` is phase-blind. What remains: a
 * push in that span that picks a phase on which the word is NOT a hit finds no
 * tail, sets keep from fill and lets the start go; the frame is then missed
 * even if the push in which it completes picks the one-shot's phase again.
 * That takes noise near the code's edge (tests/test_link_cpu.py: at amplitudes
 * 8000 and 3000 in noise of sigma 8000 every one-shot frame is received at
 * every sample offset tried; at the edge amplitudes, 1000 to 1400, 2 to 17 % of
 * them are missed); it is not solved here. So, per frame: a frame of the
 * one-shot that the receiver misses has a push in that span whose absolute
 * phase is not the one-shot's.
 *
 * C >= 2 (L + N) R, so that a frame in flight and a full packet of the same
 * length fit: after a push X[keep ..) is at most (L + N) R - 1 windows (a tail
 * is not complete, so fill - t <= (L + N - 1) R, and R - 1 more are kept),
 * which leaves room for (L + N) R + 1 new ones. A packet with more new windows
 * than that overflows (the oldest windows go and `dropped` says how many).
 */
typedef struct demod_rx_cfg {
    uint8_t  sync[DEMOD_MAX_SYNC];     /* the word, sync_len symbols */
    uint32_t sync_len, max_errors;
    uint32_t frame_symbols;            /* N */
    uint32_t len_bytes, crc;           /* h; DEMOD_CRC16_CCITT_FALSE or DEMOD_CRC32_MPEG2 */
    uint32_t fec;                      /* 0 or one of the 20 modes ("Reed-Solomon outer code") */
    uint32_t max_frames;               /* rows per stream and push */
    uint32_t ring_windows;             /* C */
} demod_rx_cfg_t;

typedef struct demod_rx_frame {        /* 32 bytes */
    uint32_t stream, length;
    uint64_t window;                   /* base + hit window: stream-absolute */
    uint64_t body;                     /* byte offset of its data in the dense body array:
                                          the exclusive prefix of `length` in output order */
    uint32_t errors, reserved;         /* the hit's errors; 0 */
} demod_rx_frame_t;

typedef struct demod_rx_stream_state { /* 40 bytes, one per stream, device and host */
    uint64_t base, hold, dropped, cut_hits;
    uint32_t fill, keep;
} demod_rx_stream_state_t;

typedef struct demod_rx_summary {
    uint64_t n_frames, n_bytes;        /* emitted rows and their data bytes */
    uint64_t n_checked, n_valid;       /* rows checked and rows OK in this push, all streams */
} demod_rx_summary_t;

typedef struct demod_rx_sizes {
    uint64_t max_len;                  /* data bytes a frame can hold */
    uint64_t row_bytes;                /* B (fec 0) or Bd */
    uint64_t ring_sym_bytes;           /* one [S][C] symbol ring */
    uint64_t ring_mag_bytes;           /* one [S][C][K] power ring */
    uint64_t scan_work_bytes;          /* demod_frames_segments_workspace_size(cfg, S, S C) */
    uint64_t decode_work_bytes;        /* demod_fec_decode_workspace_size, 0 with fec 0 */
    uint64_t collect_work_bytes;       /* demod_rx_collect_workspace_size */
    uint64_t frames_bytes;             /* d_frames: S max_frames records */
    uint64_t bodies_bytes;             /* d_bodies: S max_frames max_len */
} demod_rx_sizes_t;

/* Validates the pair and fills *out. No device needed. DEMOD_BAD_ARG for a
 * NULL pointer, whatever the scan, the check or the decode refuse for the same
 * parameters (configuration, word, (L + N) R >= 2^31, row shape, K not a power
 * of two with fec, an unknown crc, len_bytes or fec), n_streams == 0 or >
 * DEMOD_MAX_SEGMENTS, max_frames == 0, n_streams * max_frames >= 2^31,
 * ring_windows < 2 (L + N) R, ring_windows >= 2^31 / n_streams or n_streams *
 * ring_windows >= 2^31. */
int demod_rx_sizes(const demod_cfg_t *cfg, const demod_rx_cfg_t *rxcfg, size_t n_streams,
                   demod_rx_sizes_t *out);

/*
 * Step 1 for every stream, from ring "in" to ring "out": two distinct [S][C]
 * symbol and [S][C][K] power arrays that the caller alternates between pushes,
 * so no copy overlaps itself. Enqueued on `stream`: two launches whatever S and
 * the counts are (copy, then state). The new windows of stream s are windows
 * d_new_first[s] .. of (d_new_sym, d_new_mag), d_new_count[s] of them, in
 * demod_segments_layout's layout; both are clamped into n_new_windows as the
 * segment tables are, and the stored fill and keep to keep <= fill <= C: no
 * content moves a read or a write outside the arrays. d_state[s] gets base,
 * dropped and fill; keep is consumed (0 afterwards); hold and cut_hits stay.
 * The scan's tables are written: d_first[s] = s C, d_count[s] = fill. Slot
 * positions at or past fill are not written. Nothing is allocated or
 * synchronised, no atomics, no floating-point operation; every output byte is
 * a function of the inputs alone. Returns DEMOD_OK once enqueued; DEMOD_BAD_ARG,
 * before any launch, for a NULL handle or pointer, ring "in" equal to ring
 * "out", n_streams == 0 or > DEMOD_MAX_SEGMENTS, ring_windows == 0, n_streams *
 * ring_windows >= 2^31, n_new_windows >= 2^31, or a misaligned d_state,
 * d_new_first, d_first (8 bytes), d_new_count, d_count or power array (4 bytes).
 */
int demod_rx_advance_async(demod_t *st, demod_rx_stream_state_t *d_state, const uint8_t *d_ring_sym_in,
                           const float *d_ring_mag_in, const uint8_t *d_new_sym, const float *d_new_mag,
                           size_t n_new_windows, const uint64_t *d_new_first,
                           const uint32_t *d_new_count, size_t n_streams, size_t ring_windows,
                           uint8_t *d_ring_sym_out, float *d_ring_mag_out, uint64_t *d_first,
                           uint32_t *d_count, void *stream);

/* Bytes of demod_rx_collect_async's d_work for n_streams streams: two 8-byte
 * words and one 4-byte word per stream, the last array rounded up to 8. 0 when
 * the configuration is invalid or n_streams is 0 or above DEMOD_MAX_SEGMENTS.
 * No device needed. */
size_t demod_rx_collect_workspace_size(const demod_cfg_t *cfg, size_t n_streams);

/*
 * Steps 3 and 4 over the check's own outputs (d_hits and d_results the scan's;
 * d_check, d_kept, d_body and d_check_summary the check's or the coded
 * check's, group = stream). Enqueued on `stream`: three launches whatever S and
 * the counts are (per stream, prefix, write). Ranks and body offsets are a
 * deterministic two-level exclusive prefix, per stream and then over the
 * streams; no atomics, no floating-point operation. d_frames is [S max_frames],
 * d_bodies [S max_frames max_len]: nothing can overflow. Stored counts are
 * clamped to max_frames, a length to max_len, and a kept entry at or above
 * max_frames is skipped. d_state[s] gets hold, keep (at most fill) and
 * cut_hits; base, dropped and fill are read. d_summary: the totals, n_checked
 * and n_valid summed over the streams (each clamped to max_frames). Written:
 * records < n_frames, body bytes < n_bytes, every byte of *d_summary and of
 * d_state[0 .. S); nothing else. d_work may hold anything on entry. Returns
 * DEMOD_OK once enqueued; DEMOD_BAD_ARG, before any launch, for what
 * demod_frames_check_async (fec 0) or demod_frames_check_coded_async refuses
 * about the shape, a NULL pointer (d_body and d_bodies excepted when max_len ==
 * 0), work_bytes below demod_rx_collect_workspace_size, or a misaligned
 * d_state, d_hits, d_results, d_check_summary, d_frames, d_summary, d_work (8
 * bytes), d_check or d_kept (4 bytes).
 */
int demod_rx_collect_async(demod_t *st, demod_rx_stream_state_t *d_state, const demod_frame_hit_t *d_hits,
                           const demod_frames_result_t *d_results, const demod_frame_check_t *d_check,
                           const uint32_t *d_kept, const uint8_t *d_body,
                           const demod_frames_check_result_t *d_check_summary, size_t n_streams,
                           size_t max_frames, size_t sync_len, size_t frame_symbols, int len_bytes,
                           int crc, int fec, demod_rx_frame_t *d_frames, uint8_t *d_bodies,
                           demod_rx_summary_t *d_summary, void *d_work, size_t work_bytes, void *stream);

/* The receiver handle: n_streams streams of one configuration and one frame
 * format. NULL on failure, *error set (what demod_rx_sizes and
 * demod_streams_create refuse; DEMOD_NO_DEVICE, DEMOD_DEVICE_ERROR). */
typedef struct demod_rx demod_rx_t;
demod_rx_t *demod_rx_create(const demod_cfg_t *cfg, const demod_rx_cfg_t *rxcfg, size_t n_streams,
                            int *error);
void demod_rx_destroy(demod_rx_t *rx);

/* Drops the stream's sample carry, re-arms cfg.lead_in and zeroes its state: a
 * frame in flight on that stream is lost, other streams are untouched. */
int demod_rx_reset(demod_rx_t *rx, size_t stream);

/* The stream's state after the last push (all 0 after create or reset). */
int demod_rx_state(const demod_rx_t *rx, size_t stream, demod_rx_stream_state_t *state);

/*
 * One packet per stream, as demod_streams_push takes them (per-stream sample
 * carry, lead-in, stereo modes, runs laid on hop boundaries). One H2D copy of
 * the staged runs (the two layout tables ride behind them) goes in; on the
 * handle's stream the detector, demod_rx_advance_async,
 * demod_frames_segments_async, the check (or the decode and the coded check)
 * and demod_rx_collect_async run; one D2H copy of the summary, the states, the
 * records and the bytes comes back into handle-owned pinned memory (32 + 40 S
 * + S max_frames (32 + max_len) bytes: max_frames is what sizes it).
 * *frames[0 .. n_frames) and *bodies[0 .. n_bytes) point into that memory and
 * stay valid until the next call on the handle; *summary is filled. Returns
 * n_frames or a negative code; on a refusal (what demod_streams_push refuses
 * about pcm and n_frames, a NULL frames, bodies or summary) nothing is consumed.
 */
int demod_rx_push(demod_rx_t *rx, const int16_t *const *pcm, const size_t *n_frames,
                  const demod_rx_frame_t **frames, const uint8_t **bodies, demod_rx_summary_t *summary);

/* ---- transmitter: frames in, the signal of many streams out ------------ */
/*
 * The other end of the receiver: frames are encoded (checked, or checked and
 * convolutionally coded) into symbols and queued per stream on the device, and
 * every pull modulates the next samples of every stream, phase-continuous,
 * with idle symbols when a queue runs dry. Integer arithmetic alone; every
 * output byte is a function of the inputs alone. This text is normative.
 *
 *   bits = demod_bits_per_symbol(K); n = cfg.n: a symbol lasts n samples (R
 *   hops). inc[t] = llround(freqs[t] / fs 2^32) & 0xFFFFFFFF for t < K, as
 *   demod_synth_fsk derives it, and 0 for K <= t < 16. lut is the generator's
 *   Q15 sine table (16384 entries), mix64 the splitmix64 finaliser and gamma =
 *   0x9E3779B97F4A7C15, all as DESIGN.md "Synthetic input" has them.
 *
 * A frame on the air is A(len) = L + Sp(len) symbols: the word, then
 *   fec == 0                 Sp = ceil(8 (h + len + c) / bits): demod_unpack_symbols
 *                            of demod_checked_frame_encode's bytes, the missing
 *                            bits of the last symbol 0;
 *   a coded mode             Sp = demod_fec_frame_symbols(.., fec): the same of
 *                            demod_fec_frame_encode's bytes, air bits that no
 *                            kept coded bit maps to 0. K must be a power of two.
 * The idle symbol of stream-absolute symbol index q is idle[q mod idle_len].
 *
 * State per stream (all 0 after create or reset): head is the symbol being
 * modulated, offset < n the sample inside it, phase = PHI(head); the symbols
 * head <= q < tail are queued in a [S][C] byte ring at q mod C (C =
 * ring_symbols). Invariant: head + (offset > 0) <= tail <= head + C. Every
 * launch clamps the tail it reads into that range and offset to n - 1; no
 * content of the state, the ring or the tables moves an access outside the
 * arrays.
 *
 * send. Group (stream) s has cnt = min(d_count[s], max_frames) records {length,
 * body} at [s][i]; the data bytes of all records lie in one dense array of
 * n_bytes bytes. body' = min(body, n_bytes - min(length, n_bytes)), and a byte
 * at or past n_bytes reads as 0. a_i = 0 and status DEMOD_TX_BAD_LENGTH when
 * length_i > max_len, else a_i = A(length_i) + gap; e_i is the inclusive prefix
 * of a over the frames 0 .. i of the call, accepted or not. A frame of valid
 * length is accepted (DEMOD_TX_OK) iff tail + e_i - head <= C, else its status
 * is DEMOD_TX_NO_ROOM: e is monotone, so the accepted frames keep their order
 * and everything behind the first NO_ROOM is NO_ROOM. An accepted frame starts
 * at start_i = tail + e_i - a_i; its A symbols go to the ring at [start_i,
 * start_i + A) and the idle symbols of those indices to the `gap` positions
 * behind them. place[s][i] = {start_i, A, OK} or {0, 0, status}. Then tail += e
 * of the last accepted frame, accepted += the frames accepted, refused += cnt -
 * that.
 *
 * modulate. Stream s gets m = min(d_count[s], stride) samples at d_pcm[s stride
 * + x], x < m; nothing is written at x >= m (stride = max_samples). With y =
 * offset + x, q = head + y / n, r = y mod n:
 *   sym(q) = ring[q mod C] & 15 when q < tail, else the idle symbol of q;
 *   PHI(q) = phase + n sum_{head <= j < q} inc[sym(j)]  mod 2^32;
 *   ph     = PHI(q) + r inc[sym(q)]                      mod 2^32;
 *   tone   = (amplitude lut[ph >> 18] + 16384) >> 15;
 *   d      = mix64(mix64(seed + (s + 1) gamma) + (head n + y + 1) gamma);
 *   u      = the sum of d's four 16-bit fields;
 *   noise  = ((u - 131070) sigma 113512) >> 32   (int64, arithmetic shift);
 *   sample = tone + noise clamped to int16.
 * Afterwards, with y_end = offset + m: head' = head + y_end / n, offset' = y_end
 * mod n, phase' = PHI(head'), tail' = max(tail, head' + (offset' > 0)); when
 * that raises the tail (the pull ends inside an idle symbol past the queue),
 * the idle symbol of head' is stored at ring[head' mod C]: it is queued now,
 * and the next pull reads it there like any other.
 * The phase is continuous across symbols, pulls and underflow into idle, and
 * the noise depends on the stream and the stream-absolute sample alone: the
 * samples of a stream are the same bytes whatever the pull sizes are.
 */
#define DEMOD_TX_OK          0
#define DEMOD_TX_BAD_LENGTH  1   /* length > max_len */
#define DEMOD_TX_NO_ROOM     2   /* the ring cannot take the frame (or one before it) */

typedef struct demod_tx_cfg {          /* 184 bytes, no padding */
    uint8_t  sync[DEMOD_MAX_SYNC];     /* the word, sync_len symbols, each < K */
    uint32_t sync_len;                 /* L, 1 .. DEMOD_MAX_SYNC */
    uint32_t len_bytes, crc;           /* h; DEMOD_CRC16_CCITT_FALSE or DEMOD_CRC32_MPEG2 */
    uint32_t fec;                      /* 0 or one of the 20 modes ("Reed-Solomon outer code") */
    uint32_t max_len;                  /* <= min(256^h - 1, DEMOD_MAX_FRAME_PAYLOAD) */
    uint32_t gap;                      /* idle symbols behind each frame */
    uint8_t  idle[DEMOD_MAX_SYNC];     /* the idle pattern, idle_len symbols, each < K */
    uint32_t idle_len;                 /* 1 .. DEMOD_MAX_SYNC */
    int32_t  amplitude;                /* 0 .. 32767 */
    int32_t  sigma;                    /* 0 .. 32767, as demod_synth_fsk */
    uint32_t ring_symbols;             /* C >= A(max_len) + gap */
    uint64_t seed;
    uint32_t max_frames;               /* frames per stream and send */
    uint32_t max_samples;              /* samples per stream and pull: the stride, a multiple of 8 */
} demod_tx_cfg_t;

typedef struct demod_tx_stream_state { /* 40 bytes, one per stream, device and host */
    uint64_t head, tail, accepted, refused;
    uint32_t offset, phase;
} demod_tx_stream_state_t;

typedef struct demod_tx_record {       /* 8 bytes: one frame of a send, on the device */
    uint32_t length, body;             /* data bytes; their offset in the dense byte array */
} demod_tx_record_t;

typedef struct demod_tx_place {        /* 16 bytes */
    uint64_t start;                    /* stream-absolute symbol index of the word's first symbol */
    uint32_t symbols, status;          /* A(length); DEMOD_TX_*. start and symbols 0 unless OK */
} demod_tx_place_t;

typedef struct demod_tx_sizes {
    uint64_t max_symbols;              /* A(max_len) */
    uint64_t ring_bytes;               /* S C */
    uint64_t state_bytes;              /* S states */
    uint64_t places_bytes;             /* S max_frames places */
    uint64_t records_bytes;            /* S max_frames records */
    uint64_t bodies_bytes;             /* S max_frames max_len: the most a send's accepted data takes */
    uint64_t pcm_bytes;                /* S max_samples samples */
    uint64_t modulate_work_bytes;      /* demod_tx_modulate_workspace_size */
} demod_tx_sizes_t;

/* A(len) for the format of txcfg and K = k tones; DEMOD_BAD_ARG for a NULL
 * txcfg, k outside 2 .. DEMOD_MAX_TONES (with fec: not a power of two),
 * sync_len outside 1 .. DEMOD_MAX_SYNC or an unknown len_bytes, crc or fec;
 * DEMOD_FRAME_TOO_LARGE for len > max_len or what demod_checked_frame_size
 * refuses. No device needed. */
long long demod_tx_frame_symbol_count(const demod_tx_cfg_t *txcfg, uint32_t k, size_t len);

/* The A(len) symbols of one frame into out[0 .. cap), built from
 * demod_checked_frame_encode or demod_coded_frame_encode and
 * demod_unpack_symbols: the reference demod_tx_encode_async is held to. Returns
 * A(len), what demod_tx_frame_symbol_count refuses, DEMOD_BAD_ARG for a NULL
 * pointer or a word symbol >= k, or DEMOD_BUFFER_TOO_SMALL. No device needed. */
long long demod_tx_frame_symbols(const demod_tx_cfg_t *txcfg, uint32_t k, const uint8_t *data, size_t len,
                                 uint8_t *out, size_t cap);

/* Validates the pair and fills *out. No device needed. DEMOD_BAD_ARG for a
 * NULL pointer, an invalid configuration, K < 2, a word or idle length outside
 * 1 .. DEMOD_MAX_SYNC or a symbol of either >= K, an unknown crc, len_bytes or
 * fec, K not a power of two with fec, max_len above min(256^h - 1,
 * DEMOD_MAX_FRAME_PAYLOAD), C < A(max_len) + gap, n_streams == 0 or >
 * DEMOD_MAX_SEGMENTS, max_frames == 0, n_streams * max_frames >= 2^31,
 * n_streams * C >= 2^31, max_samples 0 or not a multiple of 8, n_streams *
 * max_samples >= 2^31, amplitude or sigma outside 0 .. 32767. */
int demod_tx_sizes(const demod_cfg_t *cfg, const demod_tx_cfg_t *txcfg, size_t n_streams,
                   demod_tx_sizes_t *out);

/*
 * send on the device. Enqueued on `stream`: two launches whatever S and the
 * counts are. Nothing is allocated or synchronised, no atomics, no
 * floating-point operation, and the handle keeps no state of the call: it can
 * be captured and replayed after the records, counts and bytes were rewritten
 * in place.
 *   plan   one wave a stream walks its records 64 at a time: the prefix e by a
 *          wave scan with a running carry, acceptance, the places; then tail,
 *          accepted and refused (tail and offset are stored clamped).
 *   write  one wave a frame; wave c of a group's min(max_frames, max(16384 / S,
 *          1)) waves takes frames c, c + wpg, ..: len || data || CRC in the
 *          wave's LDS, the CRC by the check's lane-split scheme, then lane j
 *          writes symbols j, j + 64, ..: the word, its bits of the checked
 *          frame or, coded, each coded bit m from the information bits (m >> 1)
 *          - 6 .. m >> 1 alone, and the gap's idle symbols. Consecutive bytes
 *          per wave step; a run may wrap the ring once.
 * d_state [S], d_ring [S][C], d_records and d_place [S][max_frames], d_count
 * [S], d_bytes [n_bytes] (may be NULL when n_bytes == 0). Written: places i <
 * cnt, the ring positions of the accepted frames, every byte of d_state;
 * nothing else. Returns DEMOD_OK once enqueued; DEMOD_BAD_ARG, before any
 * launch, for what demod_tx_sizes refuses, a NULL handle or pointer, n_bytes >=
 * 2^32, or a misaligned d_state, d_place (8 bytes), d_records or d_count (4
 * bytes).
 */
int demod_tx_encode_async(demod_t *st, const demod_tx_cfg_t *txcfg, demod_tx_stream_state_t *d_state,
                          uint8_t *d_ring, const demod_tx_record_t *d_records, const uint32_t *d_count,
                          const uint8_t *d_bytes, size_t n_bytes, size_t n_streams,
                          demod_tx_place_t *d_place, void *stream);

/* Bytes of demod_tx_modulate_async's d_work: one uint32_t PHI per symbol that a
 * pull can touch, [S][(n - 1 + max_samples) / n + 2]. 0 for what demod_tx_sizes
 * refuses. No device needed. */
size_t demod_tx_modulate_workspace_size(const demod_cfg_t *cfg, const demod_tx_cfg_t *txcfg,
                                        size_t n_streams);

/*
 * modulate on the device. Enqueued on `stream`: three launches whatever S and
 * the counts are; nothing is allocated or synchronised, no atomics, no
 * floating-point operation; d_work may hold anything on entry. The first call
 * on a device uploads the sine table (as demod_synth_fsk's does): make one
 * eager call before capturing.
 *   phase    one workgroup a stream, 1 to 16 waves by the symbols a pull of
 *            max_samples can touch, sums n inc[sym(q)] over the pull's symbols:
 *            every thread adds up 4 consecutive symbols, a shuffle scan joins
 *            a wave, the waves' totals meet in LDS and a running carry joins
 *            the steps (uint32: wrap-around addition is associative, so the
 *            grouping cannot matter); PHI is stored per symbol.
 *   samples  one thread per 8 samples, one 16-byte store per thread; the tail
 *            of a run whose m is not a multiple of 8 takes 2-byte stores. A
 *            thread reads PHI from d_work and its symbols from the ring.
 *   state    one thread a stream; last, because the other two read the state it
 *            replaces.
 * d_pcm is [S][max_samples], 16-byte aligned. Written: samples x < m of each
 * stream, every byte of d_state, the one ring byte above where the tail is
 * raised; nothing else outside d_work. Returns DEMOD_OK
 * once enqueued; DEMOD_BAD_ARG, before any launch, for what demod_tx_sizes
 * refuses, a NULL handle or pointer, work_bytes below
 * demod_tx_modulate_workspace_size, or a misaligned d_pcm (16 bytes), d_state
 * (8 bytes), d_count or d_work (4 bytes).
 */
int demod_tx_modulate_async(demod_t *st, const demod_tx_cfg_t *txcfg, demod_tx_stream_state_t *d_state,
                            uint8_t *d_ring, const uint32_t *d_count, size_t n_streams,
                            int16_t *d_pcm, void *d_work, size_t work_bytes, void *stream);

/* The transmitter handle: n_streams streams of one configuration and one frame
 * format; it owns the ring, the states, a detector handle for its stream and
 * device, and pinned staging. NULL on failure, *error set (what demod_tx_sizes
 * and demod_create refuse; DEMOD_NO_DEVICE, DEMOD_DEVICE_ERROR). cfg's
 * channels, channel_mode, lead_in and method must be valid, as for any handle,
 * but do not shape the signal: the output is mono. */
typedef struct demod_tx demod_tx_t;
demod_tx_t *demod_tx_create(const demod_cfg_t *cfg, const demod_tx_cfg_t *txcfg, size_t n_streams,
                            int *error);
void demod_tx_destroy(demod_tx_t *tx);

/* Zeroes the stream's state: what it had queued is lost, other streams are
 * untouched. */
int demod_tx_reset(demod_tx_t *tx, size_t stream);

/* The stream's state after the last send or pull (all 0 after create or reset). */
int demod_tx_state(const demod_tx_t *tx, size_t stream, demod_tx_stream_state_t *state);

/* The handle's device buffers, for callers that chain device stages behind a
 * pull: the [S][max_samples] samples of the last pull (*d_pcm) and the ring.
 * Either pointer may be NULL. */
int demod_tx_device_buffers(demod_tx_t *tx, const int16_t **d_pcm, const uint8_t **d_ring);

/*
 * Queues n frames. frames[0 .. n) is a dense list of demod_rx_frame_t, exactly
 * what demod_rx_push returns: stream, length and body (the offset of the data
 * in bodies[0 .. n_bytes)) are read, in any stream order. The host groups the
 * list stably by stream, one H2D copy takes counts, records and bytes in,
 * demod_tx_encode_async runs, and one D2H copy brings the places and the
 * states back; place[i] (when place is not NULL) is frame i's, in input order.
 * Returns the number accepted or a negative code. DEMOD_BAD_ARG, with nothing
 * queued, for a NULL handle or (with n > 0) frames, more than max_frames frames
 * for one stream, a stream >= S, or body + length > n_bytes; a length above
 * max_len is not a refusal (its place says DEMOD_TX_BAD_LENGTH).
 */
int demod_tx_send(demod_tx_t *tx, const demod_rx_frame_t *frames, size_t n, const uint8_t *bodies,
                  size_t n_bytes, demod_tx_place_t *place);

/*
 * The next n_frames[s] mono samples of every stream into pcm[s] (which may be
 * NULL where n_frames[s] == 0): the counts go in, demod_tx_modulate_async runs,
 * one D2H copy brings the samples and the states back. Returns the total
 * number of samples or a negative code; DEMOD_BAD_ARG, with nothing produced,
 * for a NULL pointer or n_frames[s] > max_samples.
 */
long long demod_tx_pull(demod_tx_t *tx, const size_t *n_frames, int16_t *const *pcm);

/* ---- many streams over many GPUs (config 5), RCCL ---------------------- */
/*
 * A group of `world` ranks, one per GPU, demodulating n_streams streams of one
 * configuration: rank r owns the contiguous stream shard
 * demod_group_shard(n_streams, r, world) and demodulates it on its own device;
 * RCCL (over xGMI) carries only the decoded result: an all-gather of every
 * rank's symbols (push) or ToReceiver frames (bucket). SURVEY.md §7 step 5 /
 * §8e: one process per GPU (demod_group_create: hipSetDevice to cfg->device +
 * ncclCommInitRank with rank 0's demod_group_unique_id, shared out of band),
 * or one process driving several GPUs (demod_group_create_local:
 * ncclCommInitAll). The reference fans one stream out to N receivers
 * (MulticastAudioOutput.kt:88-96); this gathers N GPUs' share of many streams.
 * Every call that gathers is a collective: every rank makes it.
 */
#define DEMOD_GROUP_ID_BYTES 128   /* sizeof(ncclUniqueId) */
typedef struct demod_group demod_group_t;

/* A fresh group id (ncclGetUniqueId) into id[DEMOD_GROUP_ID_BYTES]. */
int demod_group_unique_id(uint8_t *id);
/* Rank `rank`'s contiguous, balanced stream shard (pure arithmetic). */
int demod_group_shard(size_t n_streams, int rank, int world, size_t *first, size_t *count);
/* Bytes per rank of a bucket's gathered frames: steps x ceil(n_streams /
 * world) x demod_frame_symbols_size(symbols_per_stream, bits, 4096). */
long long demod_group_block_bytes(size_t n_streams, int world, size_t steps,
                                  size_t symbols_per_stream, int bits);
/* One rank of a multi-process group (cfg->device is its GPU). NULL on
 * failure, *error set. */
demod_group_t *demod_group_create(const demod_cfg_t *cfg, size_t n_streams, int rank, int world,
                                  const uint8_t *id, int *error);
/* Every rank in this process, rank i on devices[i]. */
demod_group_t *demod_group_create_local(const demod_cfg_t *cfg, size_t n_streams, int n_devices,
                                        const int *devices, int *error);
void demod_group_destroy(demod_group_t *g);
int demod_group_world(const demod_group_t *g);
int demod_group_local_ranks(const demod_group_t *g);   /* ranks this process drives */
int demod_group_rank_shard(const demod_group_t *g, int local, int *rank, size_t *first,
                           size_t *count);
/* The GPU ordinal of the local-th rank this process drives. */
int demod_group_rank_device(const demod_group_t *g, int local);
/* DEMOD_OK while the group is alive, else the code that killed it (see below). */
int demod_group_status(const demod_group_t *g);

/*
 * Errors (no abort(), negative codes; no hang). Every call
 * below is collective, and a rank never leaves one alone: each refusal is
 * decided from all-gathered words, so every rank returns the same code.
 * demod_group_push all-gathers [status, symbols == NULL, cap, per-stream
 * counts] before anything is consumed: an argument refusal on any rank
 * (demod_streams_push's own checks), a too-small cap or a total above INT_MAX
 * on any rank returns that code (the lowest failing rank's) on every rank with
 * nothing consumed. A push that fails on a rank after that point (device or
 * allocation failure) returns its code on every rank and leaves the group
 * dead: its communicator is aborted (ncclCommAbort), later calls return
 * DEMOD_INVALID_STATE and the caller destroys it. A collective that fails, or
 * does not finish within FSKD_GROUP_TIMEOUT_MS (default 120000: a peer process
 * died), aborts the communicator the same way and returns DEMOD_DEVICE_ERROR.
 */

/*
 * One packet per stream this process owns (a local group: all n_streams; one
 * rank of a multi-process group: its shard, pcm[i] = stream first + i), each
 * demodulated as demod_streams_push does (per-stream carry and lead-in).
 * Every stream's count is gathered first, then every rank's symbols; on
 * return, on every rank, symbols[] holds all n_streams streams' symbols
 * (stream 0 first) and counts[0 .. n_streams-1] their counts. Returns the
 * total; if cap is too small, every rank returns DEMOD_BUFFER_TOO_SMALL
 * before anything is consumed. A local group runs its ranks concurrently
 * (one host thread per GPU).
 */
int demod_group_push(demod_group_t *g, const int16_t *const *pcm, const size_t *n_frames,
                     uint8_t *symbols, size_t cap, uint32_t *counts);

/*
 * Config 5's step, device-resident, for each rank l this process drives
 * (arrays indexed by l): d_pcm[l] holds `ring` steps' batches of the rank's
 * streams, [ring][count][wps windows][n] (cfg.hop == n), the same batch in
 * each slot or a fresh one. `steps` (a multiple of ring) steps run as
 * steps / ring detector launches, ONE device framing launch over the steps'
 * symbol rows (one ToReceiver run per stream per step) and ONE RCCL
 * all-gather into d_all[l] ([world][block] bytes, rank q's block = its frames,
 * [step][stream][stride]), all enqueued on streams[l] (hipStream_t; NULL
 * array = default streams), so a caller may capture it in a HIP graph (make
 * one call of the shape outside capture first: it sizes the rank's buffers).
 * Every rank's status word is all-gathered beside the frames: a rank that
 * fails locally (a NULL d_pcm / d_all entry, a failed launch) still posts both
 * gathers, carrying its code, and returns that code; its peers learn it from
 * demod_group_wait. Returns block bytes (demod_group_block_bytes) or a
 * negative code (the shape, identical on every rank, is refused alike).
 */
long long demod_group_bucket_async(demod_group_t *g, const int16_t *const *d_pcm, size_t ring,
                                   size_t wps, size_t steps, uint8_t *const *d_all,
                                   void *const *streams);

/*
 * After buckets (or graph replays of one) on streams[l] (NULL array: default
 * streams): waits for them under the group's deadline, then returns the
 * lowest failing rank's status of the last bucket (the same on every rank),
 * DEMOD_OK, or DEMOD_DEVICE_ERROR when a collective failed or overran (the
 * group is then dead, as above).
 */
int demod_group_wait(demod_group_t *g, void *const *streams);

/* ---- ip.proto framing (ToReceiver{AudioData{bytes}}, delimited) ------- */

/* Bytes demod_frame_encode needs for a payload of len bytes. */
size_t demod_frame_size(size_t payload_len);

/* Encode varint32(len(msg)) || ToReceiver{audio_data{opus_encoded_frame =
 * payload}}. Returns bytes written, DEMOD_BUFFER_TOO_SMALL, or
 * DEMOD_FRAME_TOO_LARGE when len > DEMOD_MAX_FRAME_PAYLOAD. */
int demod_frame_encode(const uint8_t *payload, size_t len,
                       uint8_t *out, size_t cap);

/* Decode one delimited ToReceiver frame from in[0..len). On success
 * *payload points into `in`, *payload_len is its length, *consumed the
 * bytes of the whole frame; returns DEMOD_OK. Returns DEMOD_BUFFER_TOO_SMALL
 * when `in` holds only part of a frame (read more and retry),
 * DEMOD_INVALID_PACKET on malformed bytes, DEMOD_FRAME_TOO_LARGE when the
 * payload exceeds DEMOD_MAX_FRAME_PAYLOAD (network.cpp:223-227). */
int demod_frame_decode(const uint8_t *in, size_t len, const uint8_t **payload,
                       size_t *payload_len, size_t *consumed);

/* Bits per symbol used for packing: ceil(log2(k)), at least 1. */
int demod_bits_per_symbol(uint32_t k);

/* Pack n symbols MSB-first into ceil(n*bits/8) bytes. Returns bytes. */
int demod_pack_symbols(const uint8_t *symbols, size_t n, int bits,
                       uint8_t *out, size_t cap);
int demod_unpack_symbols(const uint8_t *in, size_t n, int bits,
                         uint8_t *symbols, size_t cap);

/* Frame a symbol stream into consecutive delimited ToReceiver frames,
 * each payload <= max_payload (<= DEMOD_MAX_FRAME_PAYLOAD) bytes of packed
 * symbols. Returns total bytes written. */
long long demod_frame_symbols(const uint8_t *symbols, size_t n, int bits,
                              size_t max_payload, uint8_t *out, size_t cap);

/* Bytes demod_frame_symbols writes for n symbols (0 for n = 0), or a
 * negative code for bad arguments. */
long long demod_frame_symbols_size(size_t n, int bits, size_t max_payload);

/* Device framing for many streams (config 5: each rank frames its own
 * streams before the RCCL gather). d_symbols holds n_streams x n symbols,
 * stream-major; stream s is framed exactly as demod_frame_symbols(symbols
 * of s, n, bits, max_payload, ...) would, into d_out + s * stride with
 * stride = demod_frame_symbols_size(n, bits, max_payload). Device pointers,
 * enqueued on `stream` (hipStream_t; NULL = default stream). Returns the
 * stride or a negative code. Stands in for nanopb pb_encode_delimited of
 * ToReceiver (network.cpp:389-403), one message per payload. */
long long demod_frame_streams_async(const uint8_t *d_symbols, size_t n_streams, size_t n,
                                    int bits, size_t max_payload, uint8_t *d_out,
                                    void *stream);

/* ---- ip.proto session messages ------------------ */
/* What a receiver exchanges around the audio stream: the delimited
 * ToTransmitter hello it writes when a transmitter connects on TCP 58764
 * (network.cpp:388-403; read by RemoteAudioReceiver.connect,
 * RemoteAudioReceiver.kt:60-68), and the BroadcastMessage datagrams of UDP
 * 58765 discovery (network.cpp:449-494; discovery.kt:23-97). Encoders emit
 * nanopb's bytes for the same struct; decoders return nanopb's verdict
 * (demod_session.c). Pure host byte work. */
#define DEMOD_PORT_AUDIO_RX    58764        /* ip.proto:28-31 (TCP) */
#define DEMOD_PORT_DISCOVERY   58765        /* ip.proto:5-7 (UDP) */
#define DEMOD_BROADCAST_MAGIC  0x2C5DA044u  /* ip.proto:10, network.cpp:448 */
#define DEMOD_INFO_STRING_CAP  128          /* char[128] strings, ip.pb.h:20,23 */
#define DEMOD_MAX_DECODED_FRAME 11520       /* AUDIO_BUFFER_SIZE, playback.cpp:10,193 */

/* oneof member tags returned by the decoders */
#define DEMOD_MSG_NONE                 0
#define DEMOD_MSG_DISCOVERY_REQUEST    2  /* BroadcastMessage.discovery_request */
#define DEMOD_MSG_DISCOVERY_RESPONSE   3  /* BroadcastMessage.discovery_response */
#define DEMOD_MSG_RECEIVER_INFORMATION 1  /* ToTransmitter.receiver_information */
#define DEMOD_MSG_RECEIVER_ERROR       2  /* ToTransmitter.error */

typedef struct {                  /* DiscoveryResponse, ip.pb.h:17-24 */
    uint32_t protocol_version;    /* 1 in the firmware (network.cpp:374) */
    uint64_t mac_address;         /* 6 MAC bytes, byte i at bits 8i (network.cpp:360-363) */
    char device_name[DEMOD_INFO_STRING_CAP];   /* NUL-terminated, <= 127 bytes */
    int currently_streaming;
    char opus_version[DEMOD_INFO_STRING_CAP];  /* NUL-terminated, <= 127 bytes */
} demod_discovery_t;

typedef struct {                  /* ReceiverInformation, ip.pb.h:55-59 */
    demod_discovery_t discovery_data;
    uint32_t max_encoded_frame_size;   /* 4096 in the firmware (network.cpp:392) */
    uint32_t max_decoded_frame_size;   /* 11520 in the firmware (network.cpp:393) */
} demod_receiver_info_t;

typedef struct {                  /* ReceiverError, ip.pb.h:61-64 */
    int audio_underflow;
    int audio_decode_error;
} demod_receiver_error_t;

/* BroadcastMessage{magic_word = DEMOD_BROADCAST_MAGIC, discovery_request =
 * true}, the datagram a transmitter broadcasts (discovery.kt:44-48).
 * Returns bytes written or DEMOD_BUFFER_TOO_SMALL. */
int demod_broadcast_request_encode(uint8_t *out, size_t cap);

/* BroadcastMessage{magic_word, discovery_response = *d}, the receiver's
 * unicast answer (network.cpp:356-378,486-492). Returns bytes written,
 * DEMOD_BUFFER_TOO_SMALL, or DEMOD_BAD_ARG for an unterminated string. */
int demod_broadcast_response_encode(const demod_discovery_t *d, uint8_t *out, size_t cap);

/* Decode one datagram as BroadcastMessage. Returns the oneof member
 * (DEMOD_MSG_NONE / _DISCOVERY_REQUEST / _DISCOVERY_RESPONSE) with *magic
 * set (and *resp filled for a response; resp may be NULL), or
 * DEMOD_INVALID_PACKET where nanopb's pb_decode fails. A receiver answers
 * exactly when this returns DEMOD_MSG_DISCOVERY_REQUEST and *magic ==
 * DEMOD_BROADCAST_MAGIC (network.cpp:473-485). */
int demod_broadcast_decode(const uint8_t *in, size_t len, uint32_t *magic,
                           demod_discovery_t *resp);

/* Length-delimited ToTransmitter{receiver_information = *info}: the hello
 * (network.cpp:388-403). Returns bytes written, DEMOD_BUFFER_TOO_SMALL or
 * DEMOD_BAD_ARG. */
int demod_hello_encode(const demod_receiver_info_t *info, uint8_t *out, size_t cap);

/* Length-delimited ToTransmitter{error = *e} (ip.proto:41-44,61-66). */
int demod_receiver_error_encode(const demod_receiver_error_t *e, uint8_t *out, size_t cap);

/* Decode one length-delimited ToTransmitter from in[0..len) (the
 * transmitter side, RemoteAudioReceiver.kt:60). Returns the oneof member
 * (DEMOD_MSG_NONE / _RECEIVER_INFORMATION / _RECEIVER_ERROR), filling *info
 * or *err (either may be NULL) and *consumed; DEMOD_BUFFER_TOO_SMALL when
 * only part of the message is in `in`; DEMOD_INVALID_PACKET where nanopb's
 * pb_decode_delimited fails. */
int demod_to_transmitter_decode(const uint8_t *in, size_t len, demod_receiver_info_t *info,
                                demod_receiver_error_t *err, size_t *consumed);

/* ---- synthetic PCM (benchmarks / tests) -------------------------------- */

/* Device generator of the seeded FSK test signal (DESIGN.md §Synthetic
 * input): windows w0 .. w0+W-1 of the stream, cfg->n mono samples each,
 * contiguous, symbols uniform
 * over cfg->k, amplitude `amplitude`, Irwin–Hall noise of std `sigma`.
 * d_pcm / d_symbols are device pointers on device cfg->device (checked:
 * DEMOD_BAD_ARG for memory of another device); enqueued on `stream`. The
 * sine table is uploaded to each device once per process: a
 * hipDeviceReset() while the library is loaded is not supported. */
int demod_synth_fsk(const demod_cfg_t *cfg, uint64_t seed, uint64_t w0,
                    size_t n_windows, int amplitude, int sigma, int16_t *d_pcm,
                    uint8_t *d_symbols, void *stream);

/* Read-only reference stream (probes): reads n_bytes (a multiple of 8192,
 * 16-byte aligned) of device memory with the detector kernels' access
 * pattern (8 KiB per wave, coalesced 16 B/lane non-temporal loads) and
 * discards it, enqueued on `stream`. A reference point for probes, not a
 * ceiling: the detector kernels measure slightly above it. */
int demod_read_ceiling_async(const void *d_buf, size_t n_bytes, void *stream);

/* ---- misc -------------------------------------------------------------- */
const char *demod_strerror(int error);   /* mirrors opus_strerror */
const char *demod_version_string(void);  /* mirrors opus_get_version_string */

#ifdef __cplusplus
}
#endif
#endif /* FSKDEMOD_DEMOD_H */
