// demod_internal.h — the contract between the C-ABI host layer and the
// kernels: constants, parameter structs and launch declarations. No device
// code (kernel_ops.h, rescue_ops.h, rescue_rows.h, lane_ops.h, frame_rows.h hold it).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct demod_acquire_result;  // include/demod.h
struct demod_frames_result;
struct demod_frame_hit;
struct demod_frame_check;
struct demod_frames_check_result;
struct demod_frame_decode;
struct demod_frame_rs;
struct demod_frame_erase;
struct demod_rx_stream_state;
struct demod_rx_frame;
struct demod_rx_summary;
struct demod_tx_stream_state;
struct demod_tx_record;
struct demod_tx_place;

namespace fskd {

constexpr int kSeg = 64;              // samples per lane segment
constexpr int kTileSamples = 64 * kSeg;  // samples one wave owns per tile (8 KiB)
constexpr int kWavesPerBlock = 4;  // residue kernel: 4-wave blocks share the rotation table
// Plain and fold kernels: 2-wave blocks. Same 16 waves per CU as 4-wave blocks
// (LDS-limited for the plain bank), but a block's LDS and slots free up as
// soon as its 2 waves finish: K = 2 330.7 -> 322.8 us, plain K = 8 461.7 ->
// 450.0 us, fold K = 8 350.6 -> 346.5 us (profiles/round1/probe_wpb.log).
constexpr int kPlainWPB = 2;
constexpr int kLdsSegStride = 144;    // bytes: 128 B segment + 16 B pad (conflict-free b128 reads)
constexpr int kLdsWaveBytes = 64 * kLdsSegStride;
constexpr int kMaxTones = 16;
constexpr int kFoldSlideSegs = 80;    // fold.hip fold_slide_kernel: segments per tile (10 KiB)
constexpr int kMaxDevices = 64;       // device ordinals the module tables cover
// the rescue's pass 0 by the fold (plan.h fold64) for fold plans up to this K
// (above, its code cost the fold kernels an occupancy step: K = 14, 4 -> 3)
constexpr int kFold64MaxK = 12;

// Uniform per-launch parameters (kernarg -> SGPRs).
struct GoertzelParams {
    const int16_t *pcm;      // window w starts at pcm + w*hop
    long long n_windows;
    long long hop;           // samples, multiple of 8
    int log2g;               // lanes per window = 2^log2g = n / 64
    int k;                   // tones
    const float4 *rot;       // [k][g] {Ar, Ai, Br, Bi} rotation of each lane segment
    uint8_t *sym;            // [n_windows]
    float *mag;              // [n_windows][k] or nullptr
    float coef[kMaxTones];   // 2 cos(w_k); reinsch: lambda_k = 2 cos(w_k) - 2 sgn_k
    float sgn[kMaxTones];    // reinsch: sign of cos(w_k) (+1 / -1)
    int reinsch;             // goertzel.hip: Reinsch-modified recurrence (tones near 0 / fs/2)
    int dcls;                // residue.hip: compile-time slot -> class pattern (DC, 0 = LDS class file)
    unsigned long long perm; // DCLS / F16: nibble s = the host's index of tone slot s
    int f16;                 // fold.hip: fold by 16 (K = 8, four tones each on Z0 / Z8)
    int zcls[kMaxTones];     // residue.hip: residue class (0..3) tone k reads
    int xcd_swizzle;         // 1: blocks b, b+8, b+16.. (one XCD) take adjacent tiles
    // goertzel.hip SLIDE (n = 1024, hop = 64 H < n): a tile is 64 contiguous
    // segments shared by slide_wt windows (0: off)
    int slide_wt;
    // 1: overlapping windows (hop < n) share lines between tiles, so the loads
    // keep them in L2 (plain policy); 0: each byte is read once (nt)
    int cached;
    // write-back bursts (wb_burst): 0 = none, else the number of bursts per
    // XCD in this launch
    int wb_bursts;
    // in-kernel decision rescue (the direct Goertzel-family kernels at n =
    // 1024): flagged windows are re-decided by their own row instead of a
    // rescue launch; rcoef = 2 cos(2 pi f_k / fs) in double, the caller's tone
    // order
    int rescue_inline;
    double rcoef[kMaxTones];
    // rescue_rows' pass 0 by the fold (plan.h fold64; plain-bank plans on
    // multiples of 8 bins read it at run time)
    int fold64;
    // rescue_rows' tables: rot64 = [k][16][4] {Ar, Ai, Br, Bi} in double (the
    // caller's tone order), pass 0's chain coefficients c[k] (= rcoef[k]
    // except by the fold, plan.h fold64), then rcoef[k] again (the exact
    // chains', read with a per-lane index);
    // pass 0 leaves a row to the exact chain when margin^2 < t2e64 E P_max;
    // t2e64 = 0: every flagged row takes the exact chain
    const double *rot64;
    double t2e64;
    // decision rescue (rescue.hip): ambiguity test constants.
    // Stage 1 (every window, no per-sample work): the int16 worst case
    // Q >= NE, threshold amb_tq sqrt(P_max), amb_tq = tau sqrt(Q); 0: no
    // flagging. Stage 2 (only rows stage 1 flags): the window's own energy,
    // threshold^2 = amb_t2e E P_max with E the detector's energy sum (plain
    // bank / residue: sum x^2, amb_t2e = tau^2 n; fold: sum xf^2 of the folded
    // window, tau^2 n / 8), floor amb_t2e E / 16.
    float amb_tq;
    float amb_floor;         // stage 1: 0 < P_max < amb_floor is ambiguous
    float amb_t2e;
    // fold detector: stage 2's energy is E_eff = (sqrt(sum xf^2) + amb_d)^2,
    // amb_d the double oracle's own error (which scales with the RAW window)
    // in units of the folded window's norm (error_model.cpp)
    float amb_d;
};

// Decision rescue. A detector's fp32 tone powers carry an
// error that error_model.cpp BOUNDS, from the kernel's own operation sequence
// and fp32 constants (round 5; no measured constant):
// |sqrt(P_k) - |X_k|| <= rho_det sqrt(E), and the double oracle's
// |sigma(P_ref,k) - |X_k|| <= rho_ref sqrt(sum x^2). A window whose fp32
// top-2 margin satisfies (P_max - P_2nd)^2 >= t2e E_eff P_max (t2e = 16
// (bound)^2) has sqrt P_max - sqrt P_2nd above twice both bounds, so its fp32
// argmax is the oracle's; every other window (and P_max == 0 with energy) is
// marked ambiguous and the rescue (rescue_rows in the detector, or
// rescue_kernel) re-decides it with the definition's double-precision
// arithmetic (bit-identical to oracle/fsk_oracle.c). The test runs in two
// stages: E_eff <= E_max for int16 input, so a window whose margin clears
// the threshold at E_max clears the exact test too and no per-sample work is
// spent on it (stage 1, amb_tq / amb_floor); only rows stage 1 flags compute
// their energy (stage 2), so quiet input (dithered silence, idle-channel
// noise) is not flagged wholesale.
// P_max == 0 (every fp32 tone power exactly zero) is a stage-1 candidate and
// ambiguous when the window's energy is not zero: input with no energy at the
// tones (a fold detector's folded window that cancels to a constant, say)
// leaves the oracle's double powers at its own rounding noise, whose argmax
// only its own arithmetic reproduces (round 4: tests/test_gpu_error_model.py
// test_rescued_decisions_every_window found one such window of clipped
// square waves on the fold-slide path). Digital silence (zero energy) is
// decided as a tie (tone 0) without a rescue, as the oracle's exact zeros are.
constexpr uint8_t kSymAmbiguous = 0x80;

// Full-spectrum detector (fft.hip), n = 1024.
struct FftParams {
    const int16_t *pcm;
    long long n_windows;
    long long hop;           // samples, even
    int k;
    int xcd_swizzle;
    const float *tw512;      // [512][2]  e^{-2 pi i m / 512}
    const float *tw1024;     // [512][2]  e^{-2 pi i k / 1024}
    const int *bins;         // [k] tone bins round(f n / fs), device
    int slot[kMaxTones];     // fft_quad_slot(bin) of each tone (quad2 register pick)
    // tones only: bit jb set = the post-pass pair block jb (pairs 2 jb and
    // 2 jb + 1 of every lane) holds some tone bin; 0xFF: every block (the
    // full post-pass, stage 2's energy by Parseval of the bin powers), else
    // only those blocks (PICK 2) and stage 2's energy n sum x^2 from the
    // samples (fft_quad_pmask; FSKD_FFT_PMASK=0: every block, measurement)
    unsigned pmask;
    uint8_t *sym;
    float *mag;              // [n_windows][k] or nullptr
    float *spec;             // [n_windows][513] or nullptr
    float amb_tq;            // decision rescue, as GoertzelParams (stage 2:
    float amb_floor;         // E = 2 x the window's 513 bin powers >= n sum x^2,
    float amb_t2e;           // Parseval, amb_t2e = tau^2)
    int rescue;            // 1: flagged windows are re-decided in the kernel (rescue_fft.h)
    const double *rtw;       // rescue: [1023] (cos, sin), stage len at len / 2 - 1 + j
    // the rescue's first pass (rescue_fft_seg, tones only): the tone bins'
    // powers in double by segments, rot64 = [k][16][4] {Ar, Ai, Br, Bi} at the
    // bins' frequencies, then 2 cos(2 pi b_k / n); t2e64 = 0: every flagged
    // window takes the double FFT
    const double *rot64;
    double t2e64;
    int fold64;              // rot64 by the fold (plan.h; every tone bin a multiple of 8)
};

// rescue.hip: re-decides every window whose symbol carries kSymAmbiguous.
struct RescueParams {
    const int16_t *pcm;      // window w at pcm + w * hop (the batch's first window)
    long long n_windows;
    long long hop;
    int n;
    int k;
    uint8_t *sym;
    int sym_aligned4;        // sym is 4-byte aligned: dword scans
    float *mag;              // [n_windows][k] or nullptr
    double coef[kMaxTones];  // Goertzel: 2 cos(2 pi f_k / fs), the caller's tone order
    // n = 1024 (round 5): the first pass by segments (rescue_rows pass 0's
    // arithmetic and tables) before the exact chains; t2e64 = 0: exact only;
    // fold64: 1 = by the fold (rescue_rows_fold0's arithmetic), 2 = by the
    // residue fold (rescue.hip seg_residue_window; plan.h)
    const double *rot64;
    double t2e64;
    int fold64;
};
hipError_t launch_rescue(const RescueParams &p, hipStream_t s);

struct SynthParams {
    uint64_t seed;
    uint64_t w0;             // index of the first generated window in the stream
    long long n_windows;
    int n;                   // samples per window (multiple of 8)
    int k;
    int amplitude;
    int sigma;
    int16_t *pcm;
    uint8_t *sym;
    uint32_t inc[kMaxTones];  // phase increment per sample, 2^32 / cycle
};

// Detectors (the kernels behind DEMOD_METHOD_*).
constexpr int kDetGoertzel = 1;  // goertzel.hip: 64-sample lane segments
constexpr int kDetFft = 2;       // fft.hip: 1024-point real FFT, argmax over tone bins
constexpr int kDetFolded = 3;    // fold.hip: Goertzel on the N/8-folded window
constexpr int kDetResidue = 4;   // residue.hip: per-residue-class folding (any integer bins)

hipError_t launch_detector(int detector, const GoertzelParams &p, hipStream_t s);
// residue.hip: rotation table is [k][g][2] float4 {C1, C2}, {C3, C4}
const void *residue_kernel_ptr(int k, int log2g, int dcls = 0, bool nt = true);
size_t residue_lds_bytes(int k, int log2g);
int tile_grid(long long n_windows, int log2g, int wpb = kWavesPerBlock, int wins_per_tile = 0);
hipError_t synth_prepare();  // upload the sine table to the current device (once, locked)
hipError_t launch_synth(const SynthParams &p, hipStream_t s);
hipError_t launch_read_ceiling(const int16_t *p, long long n_bytes, hipStream_t s);
hipError_t launch_fft_quad(const FftParams &p, hipStream_t s);  // 16 lanes / window (fft_quad.hip)
unsigned fft_quad_pmask(const int *bins, int k);  // FftParams::pmask of a tone plan
int fft_quad_slot(int bin);  // where fft_quad keeps |X[bin]|^2: 2 (16 j + t) + half, or 512 / 513 (bins 0 / 512)
// ip.proto framing of [n_streams][n] symbols, one frame run per stream (frame_gpu.hip)
long long frame_streams_size(long long n, int bits, long long max_payload, unsigned *per,
                             unsigned *full, int *frames);
hipError_t launch_frame_streams(const uint8_t *d_sym, long long n_streams, long long n, int bits,
                                long long max_payload, uint8_t *d_out, hipStream_t s);

// acquire.hip: symbol timing and sync word over a batch's outputs
constexpr int kAcqTile = 1024;       // windows per workgroup tile (DEMOD_ACQUIRE_TILE)
constexpr int kAcqMaxBlocks = 1024;  // the scan's grid: min(tiles, this)
struct AcquireParams {
    const uint8_t *sym;      // [n_windows]
    const float *mag;        // [n_windows][k]
    long long n_windows;
    long long per_phase;     // J = n_windows / phases
    int phases;              // R = n / hop, a power of two <= 64
    int k;
    int sync_len;
    unsigned max_errors;
    unsigned long long cap;
    uint8_t *out;            // [cap] or nullptr (cap == 0)
    ::demod_acquire_result *res;
    double *part;            // d_work: [grid][phases] per-block phase sums
    unsigned long long *first;  // d_work: [grid][phases] (w << 8 | errors), ~0: no match
    int grid;                // set by launch_acquire
    uint8_t sync[64];
};
int acquire_grid(long long n_windows);
hipError_t launch_acquire(AcquireParams p, hipStream_t s);

// acquire_segments.hip: the same acquisition over S segments of a batch, each
// treated as a batch of its own. d_work is a header written by the plan launch
// (per segment: clamped first and count, first tile, tiles) followed by one
// partial and one first-match word per phase per tile.
struct AcquireSegParams {
    const uint8_t *sym;               // [n_windows]
    const float *mag;                 // [n_windows][k]
    const unsigned long long *seg_first;  // [n_segments], device, as the caller wrote it
    const unsigned *seg_count;        // [n_segments]
    long long n_windows;              // Wb
    unsigned n_segments;
    unsigned budget;                  // tiles the workspace holds
    int phases;                       // R
    int k;
    int sync_len;
    unsigned max_errors;
    unsigned long long cap;
    uint8_t *out;                     // [n_segments][cap] or nullptr (cap == 0)
    ::demod_acquire_result *res;      // [n_segments]
    // d_work
    unsigned long long *w_first;      // [n_segments] min(first, Wb)
    unsigned *w_count;                // [n_segments] min(count, Wb - first')
    unsigned *w_tile0;                // [n_segments] tiles of the segments before it
    unsigned *w_tiles;                // [n_segments] 0: a short segment
    unsigned *w_total;                // [1] tiles of the call
    double *part;                     // [budget][phases]
    unsigned long long *first;        // [budget][phases] (w << 8 | errors), ~0: no match
    uint8_t sync[64];
};
// Bytes of the header for S segments, and of one tile's words (8-byte multiples).
constexpr size_t acquire_seg_header_bytes(size_t S) { return (20 * S + 4 + 7) / 8 * 8; }
constexpr size_t acquire_seg_tile_bytes(size_t R) { return 16 * R; }
// The pointers into d_work, for both segmented scans. The header: first'[S]
// (8 bytes each), then count', first tile and tiles [S] and the call's total
// (4 bytes each); then the tiles' words, which begin with part and first
// [budget][R] (acquire_frames_segments.hip's count and offs follow them).
inline void carve_seg_header(AcquireSegParams &p, void *d_work, size_t n_segments, size_t budget, size_t R)
{
    unsigned char *w = static_cast<unsigned char *>(d_work);
    p.w_first = reinterpret_cast<unsigned long long *>(w);
    p.w_count = reinterpret_cast<unsigned *>(w + 8 * n_segments);
    p.w_tile0 = p.w_count + n_segments;
    p.w_tiles = p.w_tile0 + n_segments;
    p.w_total = p.w_tiles + n_segments;
    p.part = reinterpret_cast<double *>(w + acquire_seg_header_bytes(n_segments));
    p.first = reinterpret_cast<unsigned long long *>(p.part + budget * R);
}
hipError_t launch_acquire_segments(const AcquireSegParams &p, hipStream_t s);

// acquire_frames.hip: every sync-word hit on the acquired phase, in window
// order, with fixed-length payloads. d_work, for T = ceil(n_windows / kAcqTile)
// tiles: part and tail [kAcqMaxBlocks][R] (8 bytes each), then the chosen
// phase's exclusive prefix of hits [T] (4 bytes each, padded to 8), then the
// complete hits per tile and phase [T][R] (4 bytes each, padded to 8).
struct FramesParams {
    const uint8_t *sym;      // [n_windows]
    const float *mag;        // [n_windows][k]
    long long n_windows;
    long long per_phase;     // J = n_windows / phases
    long long frame_symbols; // N
    int phases;              // R
    int k;
    int bits;                // demod_bits_per_symbol(k)
    int sync_len;            // L >= 1
    unsigned max_errors;
    unsigned long long max_frames;
    ::demod_frame_hit *hits;     // [max_frames] or nullptr (max_frames == 0)
    uint8_t *payload;            // [max_frames][N] or nullptr
    uint8_t *packed;             // [max_frames][ceil(N bits / 8)] or nullptr
    ::demod_frames_result *res;
    double *part;                // d_work: [grid][phases] per-block phase sums
    unsigned long long *tail;    // d_work: [grid][phases] lowest incomplete hit (w << 8 | errors), ~0: none
    unsigned *offs;              // d_work: [tiles] hits of the chosen phase in the tiles before
    unsigned *count;             // d_work: [tiles][phases] complete hits
    int grid;                    // set by launch_frames
    uint8_t sync[64];
};
constexpr size_t frames_work_bytes(size_t tiles, size_t R)
{
    return (size_t)16 * kAcqMaxBlocks * R + (tiles + 1) / 2 * 8 + (tiles * R + 1) / 2 * 8;
}
hipError_t launch_frames(FramesParams p, hipStream_t s);

// acquire_frames_segments.hip: the frame scan over S segments of a batch, each
// treated as a batch of its own. d_work is acquire_segments.hip's header
// (written by its plan launch, launch_acquire_seg_plan) followed, for the
// budget's B tiles, by part [B][R] (8 bytes each), tail [B][R] (8 bytes: a
// tile's lowest incomplete hit per phase, in seg.first), count [B][R] (4 bytes:
// complete hits) and offs [B] (4 bytes: the chosen phase's hits in the
// segment's tiles before), each array padded to 8 bytes.
struct FrameSegParams {
    AcquireSegParams seg;        // tables, header, part, first (= tail), sync; cap, out and res unused
    long long frame_symbols;     // N
    int bits;                    // demod_bits_per_symbol(k)
    unsigned long long max_frames;
    ::demod_frame_hit *hits;     // [n_segments][max_frames] or nullptr (max_frames == 0)
    uint8_t *payload;            // [n_segments][max_frames][N] or nullptr
    uint8_t *packed;             // [n_segments][max_frames][ceil(N bits / 8)] or nullptr
    ::demod_frames_result *res;  // [n_segments]
    unsigned *count;             // d_work: [budget][phases]
    unsigned *offs;              // d_work: [budget]
};
// Bytes of the words of B tiles, and the largest B that `bytes` hold.
constexpr size_t frames_seg_tiles_bytes(size_t B, size_t R)
{
    return 16 * B * R + (B * R + 1) / 2 * 8 + (B + 1) / 2 * 8;
}
constexpr size_t frames_seg_budget(size_t bytes, size_t R)
{
    size_t B = bytes / (20 * R + 4);   // no padding: an upper bound
    while (B > 0 && frames_seg_tiles_bytes(B, R) > bytes) --B;
    return B;
}
void launch_acquire_seg_plan(const AcquireSegParams &p, hipStream_t s);
hipError_t launch_frames_segments(const FrameSegParams &q, hipStream_t s);

// frames_check.hip: length, CRC and overlap of the rows a frame scan wrote
// (group g owns rows g max_frames + i, i < min(res[g].n_written, max_frames)).
// No workspace: select reads what check stored in `check`, body what select
// stored in `kept` and `summary`.
constexpr int kCrcPowBits = 13;           // a row's header and data are below 2^13 bytes
struct FramesCheckParams {
    const ::demod_frame_hit *hits;        // [n_groups][max_frames]
    const uint8_t *packed;                // [n_groups][max_frames][row_bytes]
    const ::demod_frames_result *res;     // [n_groups]
    unsigned n_groups;
    unsigned max_frames;                  // n_groups * max_frames < 2^31
    unsigned row_bytes;                   // B = ceil(N bits / 8)
    unsigned max_len;                     // B - len_bytes - crc_bytes <= DEMOD_MAX_FRAME_PAYLOAD
    int len_bytes;                        // h: 1 or 2
    int crc_bytes;                        // c: 2 or 4
    unsigned poly, init;                  // in the top 8 c bits of the word
    unsigned xpow8[kCrcPowBits];          // x^(8 2^j) mod P, as the register
    int bits;                             // demod_bits_per_symbol(k)
    int phases;                           // R
    int sync_len;                         // L
    int fec_depth;                        // 0: S = ceil(8 n / bits); DEMOD_FEC_DEPTH: the coded span
    int fec;                              // 0 or the coded mode (fec_map.h): the span's Sc
    int parity;                           // P of the outer code (rs_ops.h) or 0: the span is of n' bytes
    ::demod_frame_check *check;           // [n_groups][max_frames]
    uint32_t *kept;                       // [n_groups][max_frames]
    uint8_t *body;                        // [n_groups][max_frames][max_len] or nullptr
    ::demod_frames_check_result *summary; // [n_groups]
};
hipError_t launch_frames_check(const FramesCheckParams &p, hipStream_t s);
// One group's kept rows side by side, for the synchronous wrapper: out_hits[r] =
// hits[kept[r]], out_len[r] = check[kept[r]].length, r < min(summary->n_kept, max_frames).
hipError_t launch_frames_kept_rows(const ::demod_frame_hit *hits, const ::demod_frame_check *check,
                                   const uint32_t *kept, const ::demod_frames_check_result *summary,
                                   unsigned max_frames, ::demod_frame_hit *out_hits, uint32_t *out_len,
                                   hipStream_t s);

// frames_fec.hip: soft values and Viterbi decode of the rows a frame scan
// listed (groups and rows as frame_rows.h). One wave per row; wave v of the
// launch keeps the survivor words of its current row in work[v steps ..).
struct FramesFecParams {
    const ::demod_frame_hit *hits;        // [n_groups][max_frames]
    const float *mag;                     // [n_windows][k]
    const unsigned long long *first;      // [n_groups] or nullptr: every base 0
    const ::demod_frames_result *res;     // [n_groups]
    unsigned n_windows;                   // < 2^31
    unsigned n_groups;
    unsigned max_frames;                  // n_groups * max_frames < 2^31
    unsigned frame_symbols;               // N
    unsigned steps;                       // St of the mode: the greatest T with Nt(T) <= Cu
    unsigned row_bytes;                   // Bd = (St - 6) / 8
    unsigned max_len;                     // Bd - len_bytes - crc_bytes
    int len_bytes;                        // h
    int crc_bytes;                        // c
    int k, bits;                          // k = 2^bits
    int phases;                           // R
    int sync_len;                         // L; (L + N) R < 2^31
    uint8_t *rows;                        // [n_groups][max_frames][row_bytes]
    struct ::demod_frame_decode *decode;  // [n_groups][max_frames] (struct: demod.h has a function of the name)
    unsigned long long *work;             // [waves of the launch][steps]
    unsigned fec;                         // the coded mode (fec_map.h); DEMOD_FEC_CONV_K7: the map is the identity
    unsigned parity;                      // P of the outer code (rs_ops.h) or 0: the row holds n' bytes
};
hipError_t launch_frames_decode(const FramesFecParams &p, hipStream_t s);

// frames_rs.hip: the Reed-Solomon outer code over the rows a frame scan or the
// decode above wrote, in place (groups and rows as frame_rows.h). One wave
// per row, no workspace.
struct FramesRsParams {
    uint8_t *rows;                        // [n_groups][max_frames][row_bytes]
    const ::demod_frames_result *res;     // [n_groups]
    unsigned n_groups;
    unsigned max_frames;                  // n_groups * max_frames < 2^31
    unsigned row_bytes;                   // W: B, or Bd in a coded mode
    unsigned max_len;                     // the greatest len with n'(len) <= W; <= DEMOD_MAX_FRAME_PAYLOAD
    int len_bytes;                        // h
    int crc_bytes;                        // c
    int parity;                           // P: 16 or 32
    ::demod_frame_rs *rs;                 // [n_groups][max_frames]
};
hipError_t launch_frames_rs(const FramesRsParams &p, hipStream_t s);
// the same with the rows' erasure masks (include/demod.h "erasure decoding"): the kernel's second instantiation
struct FramesRsEraseParams : FramesRsParams {
    const uint64_t *erase;                // [n_groups][max_frames][ceil(row_bytes / 64)]
    ::demod_frame_erase *erec;            // [n_groups][max_frames]
};
hipError_t launch_frames_rs_erasures(const FramesRsEraseParams &p, hipStream_t s);

// frames_erasures.hip: the masks' producer over the plain rows a frame scan listed (groups and rows as
// frame_rows.h): a wave per 64 bytes of a row, no workspace.
struct FramesEraseParams {
    const ::demod_frame_hit *hits;        // [n_groups][max_frames]
    const float *mag;                     // [n_windows][k]
    const unsigned long long *first;      // [n_groups] or nullptr: every base 0
    const ::demod_frames_result *res;     // [n_groups]
    unsigned n_windows;                   // < 2^31
    unsigned n_groups;
    unsigned max_frames;                  // n_groups * max_frames < 2^31
    unsigned frame_symbols;               // N
    unsigned row_bytes;                   // B = ceil(N bits / 8)
    int k, bits;                          // k = 2^bits
    int phases;                           // R
    int sync_len;                         // L; (L + N) R < 2^31
    int level;                            // 1 .. 127
    uint64_t *erase;                      // [n_groups][max_frames][ceil(row_bytes / 64)]
};
hipError_t launch_frames_erasures(const FramesEraseParams &p, hipStream_t s);

// frames_carry.hip: the receiver's device-resident carry (include/demod.h
// "receiver"). advance moves each stream's kept windows and its new ones from
// ring "in" to ring "out" and rewrites the scan's tables; collect turns the
// check's per-stream outputs into one dense list of records and bytes.
struct RxAdvanceParams {
    ::demod_rx_stream_state *state;       // [n_streams]
    const uint8_t *ring_sym_in;           // [n_streams][ring]
    const float *ring_mag_in;             // [n_streams][ring][k]
    const uint8_t *new_sym;               // [n_new]
    const float *new_mag;                 // [n_new][k]
    const unsigned long long *new_first;  // [n_streams], device, as the caller wrote it
    const unsigned *new_count;            // [n_streams]
    unsigned long long n_new;             // < 2^31
    unsigned n_streams;
    unsigned ring;                        // C; n_streams * ring < 2^31
    int k;
    uint8_t *ring_sym_out;
    float *ring_mag_out;
    unsigned long long *seg_first;        // [n_streams] s C
    unsigned *seg_count;                  // [n_streams] fill
};
hipError_t launch_rx_advance(const RxAdvanceParams &p, hipStream_t s);

struct RxCollectParams {
    ::demod_rx_stream_state *state;       // [n_streams]
    const ::demod_frame_hit *hits;        // [n_streams][max_frames]
    const ::demod_frames_result *res;     // [n_streams]
    const ::demod_frame_check *check;     // [n_streams][max_frames]
    const uint32_t *kept;                 // [n_streams][max_frames]
    const uint8_t *body;                  // [n_streams][max_frames][max_len]
    const ::demod_frames_check_result *chk_sum;  // [n_streams]
    unsigned n_streams;
    unsigned max_frames;                  // n_streams * max_frames < 2^31
    unsigned max_len;
    int len_bytes, crc_bytes, bits, phases, sync_len, fec_depth, fec, parity;   // as FramesCheckParams
    ::demod_rx_frame *frames;             // [n_streams max_frames]
    uint8_t *bodies;                      // [n_streams max_frames max_len]
    ::demod_rx_summary *summary;
    // d_work
    unsigned long long *w_hold;           // [n_streams] hold before this push
    unsigned long long *w_bytes;          // [n_streams] emitted bytes, then their exclusive prefix
    unsigned *w_cnt;                      // [n_streams] emitted rows, then their exclusive prefix
};
constexpr size_t rx_collect_work_bytes(size_t S) { return 16 * S + (4 * S + 7) / 8 * 8; }
hipError_t launch_rx_collect(const RxCollectParams &p, hipStream_t s);

// frames_tx.hip: the transmitter's device stages (include/demod.h
// "transmitter"). encode = plan + write, modulate = phase + samples + state.
// The word and the idle pattern travel as 4-bit symbols, 16 to a 64-bit word:
// a lookup is four selects and a shift, no table in memory.
struct TxParams {
    ::demod_tx_stream_state *state;       // [n_streams]
    uint8_t *ring;                        // [n_streams][ring_symbols]
    unsigned n_streams;
    unsigned ring_symbols;                // C; n_streams * C < 2^31
    unsigned n;                           // samples per symbol, a power of two
    int log2n;
    int bits;                             // demod_bits_per_symbol(k)
    unsigned sync_len, idle_len;          // 1 .. 64
    unsigned long long sync4[4], idle4[4];
    // encode
    const ::demod_tx_record *records;     // [n_streams][max_frames]
    const unsigned *count;                // [n_streams]: frames (encode) or samples (modulate)
    const uint8_t *bytes;                 // [n_bytes]
    unsigned n_bytes;
    unsigned max_frames;                  // n_streams * max_frames < 2^31
    unsigned max_len, gap;
    int len_bytes, crc_bytes, fec;        // h, c, 0 or the coded mode (fec_map.h)
    int parity;                           // P of the outer code (rs_ops.h) or 0
    unsigned long long rs_g8[4];          // its generator's coefficients g[1 .. 32], eight to a word
    unsigned poly, init;                  // as FramesCheckParams
    unsigned xpow8[kCrcPowBits];
    ::demod_tx_place *place;              // [n_streams][max_frames]
    // modulate
    const int16_t *lut;                   // synth.hip's sine table on this device
    uint32_t inc[kMaxTones];              // 0 at and past K
    int amplitude, sigma;
    uint64_t seed;
    unsigned stride;                      // samples per stream; n_streams * stride < 2^31
    unsigned work_stride;                 // (n - 1 + stride) / n + 2
    int16_t *pcm;                         // [n_streams][stride]
    uint32_t *work;                       // [n_streams][work_stride]
};
hipError_t launch_tx_encode(const TxParams &p, hipStream_t s);
hipError_t launch_tx_modulate(const TxParams &p, hipStream_t s);
const int16_t *synth_lut_device();        // synth.hip: the table's address on the current device

}  // namespace fskd
