// error_model.cpp — the tone plan (which detector, the fp32 constants its
// kernels read) and the decision rescue's thresholds, DERIVED from those
// constants by a forward rounding-error analysis (round 5:
// VERDICT r4 item 1 — no measured constant is left in them).
//
// What is bounded. For every tone k of a window x (int16, n samples) let X_k
// be the exact DFT of x at the tone's frequency. The rescue needs, for every
// window and tone,
//   (1) |sqrt(P_fp32,k) - |X_k|| <= rho_det sqrt(E_det)   (the detector),
//   (2) |sigma(P_ref,k) - |X_k|| <= rho_ref sqrt(sum x^2)  (the double oracle,
//       oracle/fsk_oracle.c:79-96 goertzel_window_d, or its radix-2 FFT
//       oracle_fft_power), sigma(P) = sign(P) sqrt|P|,
// with E_det the energy the kernel itself sums (raw sum x^2; the fold
// detector: sum xf^2 of the window folded to n/8 samples). Then a window whose
// fp32 top-2 margin satisfies sqrt(P_1) - sqrt(P_2) > 2 (bound (1) + (2)) has
// the oracle's argmax, and (P_1 - P_2)^2 >= t2e E P_1 with t2e = 16 rho^2
// implies that margin (P_1 - P_2 <= (sqrt P_1 - sqrt P_2) 2 sqrt P_1).
//
// (1) for the Goertzel family is computed per tone from the kernel's own
// operation sequence. A lane (one 64-sample segment, or 8 folded samples, or
// one residue lane's 64 raw samples) is a linear program over its inputs:
// every node is a linear combination of earlier nodes with the kernel's fp32
// constants as exact coefficients, and every node the kernel rounds carries
// one rounding, |delta| <= u = 2^-24 (the rotation A s1 - B s2 is modelled
// with both products and the difference rounded, which covers every
// contraction the compiler may choose; int16 -> fp32 converts and the
// integer folds are exact). In long double the analysis forms, for every
// node o, its exact functional g_o (|v_o| <= ||g_o|| ||y_lane||), its
// sensitivity S_o = d(re, im)/dv_o (reverse sweep) and, for the second-order
// terms, the forward error bound of every node (one forward sweep per rounded
// node). The lane's error is then <= beta ||y_lane||,
//   beta = u sum_o |S_o| (||g_o|| + e1_o + s1_o E*)
// (e1, s1: the node's first-order error bound and sensitivity sum, E* the
// closure of the largest node error). Lanes hold disjoint samples, so
// sum_j beta_j ||y_j|| <= sqrt(sum beta_j^2) ||y|| (Cauchy-Schwarz). The
// constants' quantization (fp32 2 cos w, rotations) is not a rounding: it is
// the exact functional phi of the whole pipeline against e^{-i w pos},
// ||phi - e|| ||y||. The lane sum is a binary tree of fp32 adds; at each level
// the nodes partition the window, so the rounded values sum to at most
// ||Re phi|| ||y|| (+ errors so far) for the real parts, ||Im phi|| for the
// imaginary. The power P = re^2 + im^2 with two roundings moves sqrt P by
// at most u |X_fp32|.
// (1) for the FFT detector is structural (fft_quad.hip's levels; fft_rho).
// (2): the oracle's chain s = (x + c s1) - s2 in double injects per step an
// error e_m that is exactly an input perturbation (the chain is linear with
// x_m entering s_m with coefficient 1), so it moves X by at most ||e||_1; the
// states obey |s| <= |X| / |sin w| (and <= ||h|| ||x||), which bounds the
// power formula's rounding relative to |X|^2 (oracle_rho).
#include "plan.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

namespace fskd {

long long integer_bin(const demod_cfg_t &c, uint32_t i)
{
    const double b = c.freqs[i] * c.n / c.fs;
    const double r = std::nearbyint(b);
    if (std::fabs(b - r) > 1e-9 * std::max(1.0, b)) return -1;
    return (long long)r;
}

bool residue_eligible(const demod_cfg_t &c)
{
    for (uint32_t i = 0; i < c.k; ++i)
        if (integer_bin(c, i) < 0) return false;
    return true;
}

bool fold_eligible(const demod_cfg_t &c)
{
    for (uint32_t i = 0; i < c.k; ++i) {
        const long long b = integer_bin(c, i);
        if (b < 0 || b % 8 != 0) return false;
    }
    return true;
}

int validate_cfg(const demod_cfg_t *c)
{
    if (!c) return DEMOD_BAD_ARG;
    if (!(c->fs > 0.0) || !std::isfinite(c->fs)) return DEMOD_BAD_ARG;
    if (c->k < 1 || c->k > DEMOD_MAX_TONES) return DEMOD_BAD_ARG;
    // Goertzel tiles: n = 64 * 2^j, 64 <= n <= 4096
    if (c->n < 64 || c->n > 4096 || (c->n & (c->n - 1))) return DEMOD_BAD_ARG;
    if (c->hop < 8 || c->hop > c->n || (c->hop % 8)) return DEMOD_BAD_ARG;
    if (c->channels != 1 && c->channels != 2) return DEMOD_BAD_ARG;
    if (c->channels == 2 && (c->channel_mode < 0 || c->channel_mode > 2)) return DEMOD_BAD_ARG;
    if (c->method != DEMOD_METHOD_AUTO && c->method != DEMOD_METHOD_GOERTZEL &&
        c->method != DEMOD_METHOD_FOLDED && c->method != DEMOD_METHOD_FFT &&
        c->method != DEMOD_METHOD_RESIDUE)
        return DEMOD_UNIMPLEMENTED;
    if (c->method == DEMOD_METHOD_FFT && c->n != 1024) return DEMOD_UNIMPLEMENTED;
    if (c->lead_in > 0x7FFFFFFFu) return DEMOD_BAD_ARG;
    if (c->method == DEMOD_METHOD_FOLDED && !fold_eligible(*c)) return DEMOD_BAD_ARG;
    if (c->method == DEMOD_METHOD_RESIDUE && !residue_eligible(*c)) return DEMOD_BAD_ARG;
    for (uint32_t i = 0; i < c->k; ++i)
        if (!std::isfinite(c->freqs[i]) || c->freqs[i] < 0.0 || c->freqs[i] > c->fs / 2)
            return DEMOD_BAD_ARG;
    return DEMOD_OK;
}

void build_plan(const demod_cfg_t &c, Plan &pl)
{
    pl = Plan();
    const int g = (int)(c.n / 64);
    int lg = 0;
    while ((1 << lg) < g) ++lg;
    pl.log2g = lg;
    // AUTO: the plain bank is HBM-bound up to K = 2 and within
    // a few % of it to K = 4; beyond, fold when every tone is a multiple of 8
    // bins (K >= 3), else fold per residue class when every tone is on an
    // integer bin (K >= 5: at K = 3, 4 the plain bank measured as fast).
    // Overlapping windows at n = 1024 with hop a multiple of 64 share their
    // 64-sample segments: the plain bank computes each segment once (SLIDE,
    // goertzel.hip) and the fold detector runs its folded sums forward from
    // window to window (fold_slide_kernel, fold.hip). The
    // residue detector has no segment-shared form, so AUTO keeps the plain
    // SLIDE over it up to hop 384 (8-FSK on bins 32 + 9 i: 0.70 vs 0.90 ms at
    // hop 256, 0.63 vs 0.64 at 384, 0.58 vs 0.52 at 512).
    // FSKD_NO_SLIDE=1 (measurement switch for probes) runs the direct kernels.
    const char *no_slide_env = std::getenv("FSKD_NO_SLIDE");
    pl.slide = lg == 4 && c.hop < c.n && c.hop % 64 == 0 && !(no_slide_env && no_slide_env[0] == '1');
    pl.detector = kDetGoertzel;
    if (c.method == DEMOD_METHOD_FOLDED) pl.detector = kDetFolded;
    else if (c.method == DEMOD_METHOD_RESIDUE) pl.detector = kDetResidue;
    else if (c.method == DEMOD_METHOD_FFT) pl.detector = kDetFft;
    else if (c.method == DEMOD_METHOD_AUTO) {
        if (c.k >= 3 && fold_eligible(c)) pl.detector = kDetFolded;
        else if (!(pl.slide && c.hop <= 384) && c.k >= 5 && residue_eligible(c))
            pl.detector = kDetResidue;
    }
    for (uint32_t k = 0; k < c.k; ++k) pl.rcoef[k] = 2.0 * std::cos(2.0 * M_PI * c.freqs[k] / c.fs);
    if (pl.detector == kDetFft) {
        for (uint32_t k = 0; k < c.k; ++k) {
            long b = std::lround(c.freqs[k] * c.n / c.fs);
            pl.fft_bins[k] = (int)std::min<long>(std::max<long>(b, 0), c.n / 2);
            pl.fft_slot[k] = fft_quad_slot(pl.fft_bins[k]);
        }
    }
    // Rotation of each lane's piece into window phase, X += A s1 - B s2:
    //   Goertzel: segment j = samples [64j, 64j+64): A = e^{-jw(64j+63)}, B = e^{-jw(64j+64)}
    //   Folded:   folded samples [8j, 8j+8):         A = e^{-jw(8j+7)},   B = e^{-jw(8j+8)}
    //   Residue:  as Folded, with the class input s = (lo, hi) mapped to the
    //             complex s_c = (alpha lo + beta hi) + i gamma hi, folded into
    //             X = lo1 C1 + hi1 C2 + lo2 C3 + hi2 C4 (residue.hip):
    //             C1 = alpha A, C2 = beta A + gamma iA, C3 = -alpha B, C4 = -(beta B + gamma iB)
    //   Plain bank, Reinsch form (goertzel.hip RS; plans with a tone where
    //             |sin w| < kReinschSin): coefficient lambda = 2cos w - 2 sgn,
    //             state (s, d); X += (A - sgn B) s + sgn B d, stored as
    //             {C1, -C2} so the kernel's A s1 - B s2 form is unchanged.
    //             fp32 emulation of 64-sample chains: the 2cos(w) form reaches
    //             4-8e-5 of P at |sin w| ~ 0.01 and ~5e-6 at 0.05-0.08; the
    //             Reinsch form stays below 1e-6 at every bin.
    const bool residue = pl.detector == kDetResidue;
    const double span = (pl.detector == kDetFolded || residue) ? 8.0 : 64.0;
    constexpr double kReinschSin = 0.1;
    if (pl.detector == kDetGoertzel)
        for (uint32_t k = 0; k < c.k; ++k)
            if (std::fabs(std::sin(2.0 * M_PI * c.freqs[k] / c.fs)) < kReinschSin) pl.reinsch = true;
    // residue rho = bin mod 8 -> (class, alpha, beta, gamma); rho and 8 - rho
    // share a class (conjugates), class 0 carries (Z0, Z4)
    static const int kCls[8] = {0, 1, 3, 2, 0, 2, 3, 1};
    static const double kGam[8] = {0, 1, -1, 1, 0, -1, 1, -1};
    // Residue detector, compile-time classes (residue.hip DC): at n = 1024 and
    // K = 8 or 16, kernel tone slot s holds tone slot_tone[s] with a fixed
    // slot -> class pattern, so the kernel selects classes at compile time (no
    // LDS class file) and forms only the classes it reads; the window_sum
    // epilogue maps slots back (perm). Mode 1: K / 4 tones in every class
    // (class (s / 2) % 4; e.g. 8 tones on an odd bin spacing hit every residue
    // once); 2: half the tones in class 0 and half in class 3 (slots < K / 2
    // class 0; even spacings 2 and 6); 3: every tone in class 0; 4: every tone
    // in class 3. Other plans keep the LDS class file (mode 0).
    for (uint32_t sl = 0; sl < c.k; ++sl) pl.slot_tone[sl] = (int)sl;
    if (residue && lg == 4 && (c.k == 8 || c.k == 16)) {
        std::vector<uint32_t> by_cls[4];
        for (uint32_t k = 0; k < c.k; ++k) by_cls[kCls[integer_bin(c, k) % 8]].push_back(k);
        size_t cnt[4];
        for (int cl = 0; cl < 4; ++cl) cnt[cl] = by_cls[cl].size();
        const size_t K = c.k;
        if (cnt[0] == K / 4 && cnt[1] == K / 4 && cnt[2] == K / 4 && cnt[3] == K / 4) pl.dcls = 1;
        else if (cnt[0] == K / 2 && cnt[3] == K / 2) pl.dcls = 2;
        else if (cnt[0] == K) pl.dcls = 3;
        else if (cnt[3] == K) pl.dcls = 4;
        if (pl.dcls) {
            size_t next[4] = {0, 0, 0, 0};
            for (uint32_t sl = 0; sl < c.k; ++sl) {
                const int cl = pl.dcls == 1 ? (int)((sl / 2) % 4)
                             : pl.dcls == 2 ? (sl < K / 2 ? 0 : 3) : pl.dcls == 3 ? 0 : 3;
                pl.slot_tone[sl] = (int)by_cls[cl][next[cl]++];
                pl.perm |= (unsigned long long)pl.slot_tone[sl] << (4 * sl);
            }
        }
    }
    // Fold detector, F16 (fold.hip): n = 1024, K = 8 on multiples of 8 bins
    // with four tones on multiples of 16 (read Z0) and four on odd multiples
    // of 8 (read Z8), e.g. the survey's 8-FSK plan; slots 0-3 hold the Z0
    // tones, 4-7 the Z8 tones, and lane j of a window covers folded positions
    // 8 (j & 7) .. +7 of the N/16-sample fold.
    if (pl.detector == kDetFolded && lg == 4 && c.k == 8) {
        std::vector<uint32_t> z0, z8;
        for (uint32_t k = 0; k < c.k; ++k) ((integer_bin(c, k) / 8) % 2 ? z8 : z0).push_back(k);
        if (z0.size() == 4 && z8.size() == 4) {
            for (uint32_t sl = 0; sl < 8; ++sl) {
                pl.slot_tone[sl] = (int)(sl < 4 ? z0[sl] : z8[sl - 4]);
                pl.perm |= (unsigned long long)pl.slot_tone[sl] << (4 * sl);
            }
            pl.f16 = true;
        }
    }
    if (pl.detector != kDetFft) {
        pl.rot.assign((size_t)c.k * g * (residue ? 2 : 1), float4{});
        for (uint32_t sl = 0; sl < c.k; ++sl) {
            const uint32_t k = (uint32_t)pl.slot_tone[sl];  // rows below are kernel slots (= tones unless DCLS)
            const double w = 2.0 * M_PI * c.freqs[k] / c.fs;
            const double sg = std::cos(w) >= 0.0 ? 1.0 : -1.0;
            pl.sgn[sl] = (float)sg;
            pl.coef[sl] = (float)(2.0 * std::cos(w));
            if (pl.reinsch) {
                const double h = std::sin(0.5 * w), q = std::cos(0.5 * w);
                pl.coef[sl] = (float)(sg > 0 ? -4.0 * h * h : 4.0 * q * q);
            }
            const int rho = residue ? (int)(integer_bin(c, k) % 8) : 0;
            const double al = rho == 4 ? 0.0 : 1.0, be = rho == 4 ? 1.0 : 0.0, ga = kGam[rho];
            pl.zcls[sl] = kCls[rho];
            for (int j = 0; j < g; ++j) {
                const double pos = pl.f16 ? (double)(j & 7) : (double)j;  // F16: lanes j, j + 8 share positions
                const double a = -w * (span * pos + span - 1.0), b = -w * (span * pos + span);
                const double Ar = std::cos(a), Ai = std::sin(a), Br = std::cos(b), Bi = std::sin(b);
                if (!residue && pl.reinsch) {
                    const double C1r = Ar - sg * Br, C1i = Ai - sg * Bi;
                    pl.rot[(size_t)sl * g + j] = make_float4((float)C1r, (float)C1i, (float)(-sg * Br),
                                                             (float)(-sg * Bi));
                    continue;
                }
                if (!residue) {
                    pl.rot[(size_t)sl * g + j] = make_float4((float)Ar, (float)Ai, (float)Br, (float)Bi);
                    continue;
                }
                // iA = (-Ai, Ar)
                pl.rot[((size_t)sl * g + j) * 2] =
                    make_float4((float)(al * Ar), (float)(al * Ai), (float)(be * Ar - ga * Ai),
                                (float)(be * Ai + ga * Ar));
                pl.rot[((size_t)sl * g + j) * 2 + 1] =
                    make_float4((float)(-al * Br), (float)(-al * Bi), (float)(-(be * Br - ga * Bi)),
                                (float)(-(be * Bi + ga * Br)));
            }
        }
    }
    // the in-kernel rescue's first pass (n = 1024): per tone and lane segment
    // j the rotation of the segment's end state into the window's phase,
    // X = A s1 - B s2, A = e^{-i w (64 j + 63)}, B = e^{-i w (64 j + 64)}, in
    // double and in the caller's tone order, then the chains' coefficients
    // (the FFT detector: at its tone bins' frequencies b fs / n, with 2 cos
    // (2 pi b / n), for its own first pass, rescue_fft_seg)
    // Fold detector plans (every tone on a multiple of 8 bins) run it by the
    // fold (Plan::fold64): lane j over folded samples 8j .. 8j + 7 at the
    // exact bin (8x fewer double steps than 64 raw samples per lane per tone).
    if (c.n == 1024 && c.k >= 2) {
        const bool fft = pl.detector == kDetFft;
        // plain-bank plans at K <= 2 on multiples of 8 bins too (the survey's
        // 2-FSK), where the windows are evaluated one by one (SLIDE's rescue
        // launch shares segment states instead, cheaper at hop < n);
        // FSKD_PASS0_FOLD=0 (a test / measurement switch) keeps segments
        const char *pf_env = std::getenv("FSKD_PASS0_FOLD");
        const bool plain_fold = pl.detector == kDetGoertzel && c.k <= 2 && !pl.slide && fold_eligible(c);
        const bool off = pf_env && pf_env[0] == '0';
        pl.fold64 = (c.k <= (uint32_t)kFold64MaxK && (pl.detector == kDetFolded || fft || plain_fold) &&
                     !off) ? 1 : 0;
        for (uint32_t k = 0; fft && k < c.k; ++k)
            if (pl.fft_bins[k] % 8) pl.fold64 = 0;
        // the residue detector's plans (round 5): by the residue fold, in the
        // rescue launch (demod_api.cpp rescue_in_kernel)
        if (pl.detector == kDetResidue && !off) pl.fold64 = 2;
        const double span = pl.fold64 ? 8.0 : 64.0;
        // [k][16][4], pass 0's chain coefficients c[k], the oracle's rcoef[k]
        // (the exact chains' coefficients), then each tone's residue rho
        // (fold64 = 2)
        pl.rot64.assign((size_t)c.k * 16 * 4 + 3 * c.k, 0.0);
        for (uint32_t k = 0; k < c.k; ++k) {
            const double w = fft          ? 2.0 * M_PI * pl.fft_bins[k] / (double)c.n
                             : pl.fold64 ? 2.0 * M_PI * (double)integer_bin(c, k) / (double)c.n
                                         : 2.0 * M_PI * c.freqs[k] / c.fs;
            pl.rot64[(size_t)c.k * 64 + k] = (fft || pl.fold64) ? 2.0 * std::cos(w) : pl.rcoef[k];
            pl.rot64[(size_t)c.k * 65 + k] = pl.rcoef[k];
            if (pl.fold64 == 2) pl.rot64[(size_t)c.k * 66 + k] = (double)(integer_bin(c, k) % 8);
            for (int j = 0; j < 16; ++j) {
                const double a = -w * (span * j + span - 1.0), b = -w * (span * j + span);
                double *o = &pl.rot64[((size_t)k * 16 + j) * 4];
                o[0] = std::cos(a);
                o[1] = std::sin(a);
                o[2] = std::cos(b);
                o[3] = std::sin(b);
            }
        }
    }
}

void build_fft_tables(uint32_t n, FftTables &t)
{
    t.tw512.resize(1024);
    t.tw1024.resize(1024);
    for (int m = 0; m < 512; ++m) {
        t.tw512[2 * m] = (float)std::cos(-2.0 * M_PI * m / 512.0);
        t.tw512[2 * m + 1] = (float)std::sin(-2.0 * M_PI * m / 512.0);
        t.tw1024[2 * m] = (float)std::cos(-2.0 * M_PI * m / 1024.0);
        t.tw1024[2 * m + 1] = (float)std::sin(-2.0 * M_PI * m / 1024.0);
    }
    // the rescue's radix-2 twiddles: stage len (2 .. n), j < len / 2 at
    // len / 2 - 1 + j, each the (cos, sin) of (-2 pi / len) j exactly as
    // the double FFT of the definition evaluates it (one libm sincos of
    // the same rounded argument)
    t.rtw.resize(2 * (size_t)(n - 1));
    for (uint32_t len = 2; len <= n; len <<= 1) {
        const double ang = -(2.0 * M_PI) / (double)len;
        for (uint32_t j = 0; j < len / 2; ++j) {
            double sn, cs;
            sincos(ang * (double)j, &sn, &cs);
            t.rtw[2 * (len / 2 - 1 + j)] = cs;
            t.rtw[2 * (len / 2 - 1 + j) + 1] = sn;
        }
    }
}

// ---------------------------------------------------------------------------
// The bound engine.
namespace {

using ld = long double;
using cld = std::complex<ld>;
constexpr ld kU32 = 5.9604644775390625e-8L;             // 2^-24, fp32 unit roundoff
constexpr ld kU64 = 1.1102230246251565404236316680908e-16L;  // 2^-53
constexpr ld kPi = 3.14159265358979323846264338327950288L;

// One lane's linear program (see the file comment).
struct Lane {
    int nin;
    std::vector<std::vector<std::pair<int, ld>>> terms;
    std::vector<char> rnd;
    std::vector<ld> g;  // [node][nin]
    explicit Lane(int n) : nin(n)
    {
        terms.resize(n);
        rnd.assign(n, 0);
        g.assign((size_t)n * n, 0.0L);
        for (int i = 0; i < n; ++i) g[(size_t)i * n + i] = 1.0L;
    }
    int size() const { return (int)terms.size(); }
    // sum coef * node (node < 0: the constant 0). r: the kernel rounds the
    // result. A single term with coefficient 1 is the node itself (exact).
    int op(std::initializer_list<std::pair<int, ld>> t0, bool r)
    {
        std::vector<std::pair<int, ld>> t;
        for (const auto &e : t0)
            if (e.first >= 0 && e.second != 0.0L) t.push_back(e);
        if (t.empty()) return -1;
        if (t.size() == 1 && t[0].second == 1.0L) return t[0].first;
        const int id = size();
        terms.push_back(t);
        rnd.push_back(r ? 1 : 0);
        g.resize(g.size() + nin, 0.0L);
        ld *o = &g[(size_t)id * nin];
        for (const auto &e : t) {
            const ld *s = &g[(size_t)e.first * nin];
            for (int i = 0; i < nin; ++i) o[i] += e.second * s[i];
        }
        return id;
    }
};

struct LaneResult {
    ld beta = 0;             // |(re, im) error| <= beta ||y_lane||
    std::vector<cld> phi;    // exact functional of (re + i im) over the lane's inputs
};

// The lane-independent part of a lane (the chain, and the residue classes):
// a Lane over the samples whose outputs are the chain states. Analysed once
// per tone; every lane then applies its own rotation (Head) to the outputs.
struct Core {
    int nin = 0, nout = 0;
    std::vector<int> rounded;  // rounded node ids
    std::vector<ld> gn;        // ||g_r|| per rounded node
    std::vector<ld> a;         // [rounded][nout]: d(output q) / d(node r)
    std::vector<ld> e1, s1;    // per rounded node: first-order error bound / sensitivity sum into it
    ld e1max = 0, s1max = 0;   // over every node (outputs included)
    std::vector<ld> gout;      // [nout][nin] functionals of the outputs
    std::vector<ld> gram;      // [nout][nout]
};

Core analyze_core(const Lane &L, const std::vector<int> &outs)
{
    const int N = L.size(), nin = L.nin, no = (int)outs.size();
    Core c;
    c.nin = nin;
    c.nout = no;
    std::vector<ld> gn(N);
    for (int o = 0; o < N; ++o) {
        ld s = 0;
        for (int i = 0; i < nin; ++i) s += L.g[(size_t)o * nin + i] * L.g[(size_t)o * nin + i];
        gn[o] = std::sqrt(s);
    }
    // d(output q) / d(node) for every node (reverse sweeps)
    std::vector<ld> sens((size_t)no * N, 0.0L);
    for (int q = 0; q < no; ++q) {
        if (outs[q] < 0) continue;
        ld *sq = &sens[(size_t)q * N];
        sq[outs[q]] = 1.0L;
        for (int o = N - 1; o >= nin; --o)
            for (const auto &e : L.terms[o]) sq[e.first] += e.second * sq[o];
    }
    std::vector<ld> e1(N, 0.0L), s1(N, 0.0L), d(N, 0.0L);
    for (int r = nin; r < N; ++r) {
        if (!L.rnd[r]) continue;
        std::fill(d.begin() + r, d.end(), 0.0L);
        d[r] = 1.0L;
        for (int o = r + 1; o < N; ++o) {
            ld v = 0;
            for (const auto &e : L.terms[o])
                if (e.first >= r) v += e.second * d[e.first];
            d[o] = v;
            const ld av = std::fabs(v);
            e1[o] += av * gn[r];
            s1[o] += av;
        }
    }
    for (int o = nin; o < N; ++o) {
        c.e1max = std::max(c.e1max, e1[o]);
        c.s1max = std::max(c.s1max, s1[o]);
        if (!L.rnd[o]) continue;
        c.rounded.push_back(o);
        c.gn.push_back(gn[o]);
        c.e1.push_back(e1[o]);
        c.s1.push_back(s1[o]);
        for (int q = 0; q < no; ++q) c.a.push_back(sens[(size_t)q * N + o]);
    }
    c.gout.assign((size_t)no * nin, 0.0L);
    for (int q = 0; q < no; ++q)
        if (outs[q] >= 0)
            for (int i = 0; i < nin; ++i) c.gout[(size_t)q * nin + i] = L.g[(size_t)outs[q] * nin + i];
    c.gram.assign((size_t)no * no, 0.0L);
    for (int p = 0; p < no; ++p)
        for (int q = 0; q < no; ++q) {
            ld s = 0;
            for (int i = 0; i < nin; ++i) s += c.gout[(size_t)p * nin + i] * c.gout[(size_t)q * nin + i];
            c.gram[(size_t)p * no + q] = s;
        }
    return c;
}

// One lane: its head H is a Lane over the core's outputs (inputs 0 .. nout-1,
// so every head node's g is its coefficient vector on them) with outputs re, im.
LaneResult analyze_lane(const Core &c, const Lane &H, int ore, int oim, ld u)
{
    const int no = c.nout, N = H.size(), R = (int)c.rounded.size();
    LaneResult res;
    // head node norms through the Gram matrix
    std::vector<ld> hn(N, 0.0L);
    for (int h = no; h < N; ++h) {
        const ld *v = &H.g[(size_t)h * no];
        ld s = 0;
        for (int p = 0; p < no; ++p)
            for (int q = 0; q < no; ++q) s += v[p] * v[q] * c.gram[(size_t)p * no + q];
        hn[h] = std::sqrt(std::max(s, (ld)0));
    }
    std::vector<ld> sre(N, 0.0L), sim(N, 0.0L);
    if (ore >= 0) sre[ore] = 1.0L;
    if (oim >= 0) sim[oim] = 1.0L;
    for (int o = N - 1; o >= no; --o)
        for (const auto &e : H.terms[o]) {
            sre[e.first] += e.second * sre[o];
            sim[e.first] += e.second * sim[o];
        }
    // errors into head nodes: from core rounded nodes (through the outputs)
    // and from earlier head rounded nodes
    std::vector<ld> e1(N, 0.0L), s1(N, 0.0L), d(N, 0.0L);
    for (int h = no; h < N; ++h) {
        const ld *v = &H.g[(size_t)h * no];
        for (int r = 0; r < R; ++r) {
            ld x = 0;
            for (int q = 0; q < no; ++q) x += v[q] * c.a[(size_t)r * no + q];
            const ld ax = std::fabs(x);
            e1[h] += ax * c.gn[r];
            s1[h] += ax;
        }
    }
    for (int r = no; r < N; ++r) {
        if (!H.rnd[r]) continue;
        std::fill(d.begin() + r, d.end(), 0.0L);
        d[r] = 1.0L;
        for (int o = r + 1; o < N; ++o) {
            ld v = 0;
            for (const auto &e : H.terms[o])
                if (e.first >= r) v += e.second * d[e.first];
            d[o] = v;
            e1[o] += std::fabs(v) * hn[r];
            s1[o] += std::fabs(v);
        }
    }
    ld e1m = c.e1max, s1m = c.s1max;
    for (int h = no; h < N; ++h) {
        e1m = std::max(e1m, e1[h]);
        s1m = std::max(s1m, s1[h]);
    }
    if (u * s1m >= 0.5L) {  // never for the shipped programs; a bound that cannot close
        res.beta = HUGE_VALL;
        return res;
    }
    const ld estar = u * e1m / (1.0L - u * s1m);
    ld beta = 0;
    for (int r = 0; r < R; ++r) {
        ld xr = 0, xi = 0;
        for (int q = 0; q < no; ++q) {
            xr += sre[q] * c.a[(size_t)r * no + q];
            xi += sim[q] * c.a[(size_t)r * no + q];
        }
        beta += std::hypot(xr, xi) * (c.gn[r] + u * c.e1[r] + u * c.s1[r] * estar);
    }
    for (int h = no; h < N; ++h)
        if (H.rnd[h]) beta += std::hypot(sre[h], sim[h]) * (hn[h] + u * e1[h] + u * s1[h] * estar);
    res.beta = u * beta;
    res.phi.assign(c.nin, cld(0, 0));
    for (int q = 0; q < no; ++q) {
        const ld wr = ore >= 0 ? H.g[(size_t)ore * no + q] : 0.0L;
        const ld wi = oim >= 0 ? H.g[(size_t)oim * no + q] : 0.0L;
        for (int i = 0; i < c.nin; ++i) res.phi[i] += cld(wr, wi) * c.gout[(size_t)q * c.nin + i];
    }
    return res;
}

// fp32 Goertzel chain over x (node ids), s = fma(c, s1, x - s2): the kernels'
// plain form (goertzel.hip, fold.hip, residue.hip)
void chain_plain(Lane &L, const std::vector<int> &x, ld c, int &s1, int &s2)
{
    s1 = s2 = -1;
    for (int xi : x) {
        const int a = L.op({{xi, 1.0L}, {s2, -1.0L}}, true);
        const int s = L.op({{s1, c}, {a, 1.0L}}, true);
        s2 = s1;
        s1 = s;
    }
}

// Reinsch form (goertzel.hip RS): d' = fma(sg, d, x), d = fma(lambda, s, d'),
// s = fma(sg, s, d); the kernel keeps s in s1 and d in s2
void chain_reinsch(Lane &L, const std::vector<int> &x, ld lam, ld sg, int &s1, int &s2)
{
    int s = -1, d = -1;
    for (int xi : x) {
        const int t = L.op({{d, sg}, {xi, 1.0L}}, true);
        const int dd = L.op({{s, lam}, {t, 1.0L}}, true);
        const int sn = L.op({{s, sg}, {dd, 1.0L}}, true);
        d = dd;
        s = sn;
    }
    s1 = s;
    s2 = d;
}

// the double chain of the in-kernel rescue's first pass (contraction off):
// p = c s1, q = x + p, s = q - s2, each rounded
void chain_double(Lane &L, const std::vector<int> &x, ld c, int &s1, int &s2)
{
    s1 = s2 = -1;
    for (int xi : x) {
        const int p = L.op({{s1, c}}, true);
        const int q = L.op({{xi, 1.0L}, {p, 1.0L}}, true);
        const int s = L.op({{q, 1.0L}, {s2, -1.0L}}, true);
        s2 = s1;
        s1 = s;
    }
}

// re = rx s1 - rz s2, im = ry s1 - rw s2: both products and the difference
// rounded (every contraction the kernels' C or packed forms may take)
void rotate2(Lane &L, int s1, int s2, ld rx, ld ry, ld rz, ld rw, int &re, int &im)
{
    const int pa = L.op({{s1, rx}}, true), pb = L.op({{s2, rz}}, true);
    re = L.op({{pa, 1.0L}, {pb, -1.0L}}, true);
    const int qa = L.op({{s1, ry}}, true), qb = L.op({{s2, rw}}, true);
    im = L.op({{qa, 1.0L}, {qb, -1.0L}}, true);
}

// One tone over a window: lanes (their results and the window positions of
// their inputs), the reference frequency, the tree's levels. Returns the
// detector's bound per ||y||: (phi - e) + lanes + tree + power.
struct WindowAcc {
    int M;                   // positions
    std::vector<cld> phi;
    ld sumb2 = 0;
    explicit WindowAcc(int m) : M(m), phi(m, cld(0, 0)) {}
    void add(const LaneResult &r, const std::vector<int> &pos)
    {
        sumb2 += r.beta * r.beta;
        for (size_t i = 0; i < pos.size(); ++i) phi[pos[i]] += r.phi[i];
    }
    ld finish(ld w_ref, int levels, ld u) const
    {
        ld a2 = 0, ren = 0, imn = 0;
        for (int p = 0; p < M; ++p) {
            const cld e(std::cos(w_ref * p), -std::sin(w_ref * p));
            a2 += std::norm(phi[p] - e);
            ren += phi[p].real() * phi[p].real();
            imn += phi[p].imag() * phi[p].imag();
        }
        const ld A = std::sqrt(a2), C = std::sqrt(sumb2);
        ren = std::sqrt(ren);
        imn = std::sqrt(imn);
        ld T = 0;
        for (int l = 0; l < levels; ++l) {
            const ld bre = u * (ren + C + T), bim = u * (imn + C + T);
            T += std::hypot(bre, bim);
        }
        const ld pn = std::sqrt(ren * ren + imn * imn);
        const ld power = u * (pn + C + T);
        return A + C + T + power;
    }
};

// The double oracle's bound (2) for one tone: chain s = (x + c s1) - s2 over
// n samples, then P = (s1^2 + s2^2) - (c s1) s2 (oracle/fsk_oracle.c:79-96),
// per ||x||.
ld oracle_rho(double cd, int n)
{
    const ld u = kU64, c = cd, ac = std::fabs(c);
    // H_m = ||h[0..m]||, h the impulse response of the exact recurrence
    std::vector<ld> H(n);
    ld h1 = 0, h2 = 0, acc = 0;
    for (int m = 0; m < n; ++m) {
        const ld h = (m == 0) ? 1.0L : c * h1 - h2;
        h2 = h1;
        h1 = h;
        acc += h * h;
        H[m] = std::sqrt(acc);
    }
    ld A = 0;
    for (int m = 0; m < n; ++m) A += 2.0L * ac * (m ? H[m - 1] : 0.0L) + H[m];
    const ld k1 = u * (1.0L + 2.0L * u);
    if (k1 * A >= 0.5L) return HUGE_VALL;
    const ld chain = k1 * (A + std::sqrt((ld)n)) / (1.0L - k1 * A);
    const ld sin2 = 1.0L - c * c / 4.0L;
    const ld q = (2.0L * u + u * u) * (2.0L + ac);
    ld pw = 2.0L * std::sqrt((q * H[n - 1] * H[n - 1] + u * n) / (1.0L - u)) * (1.0L + chain);
    if (sin2 > 0) {
        const ld kap = (q / sin2 + u) / (1.0L - u);
        if (kap < 0.5L) pw = std::min(pw, kap * std::sqrt((ld)n) * (1.0L + chain));
    }
    return chain + pw;
}

// ||e(w_a) - e(w_b)|| over n positions: the oracle's frequency against the
// exact bin the fold / residue identities need
ld freq_gap(ld wa, ld wb, int n)
{
    ld s = 0;
    for (int p = 0; p < n; ++p) s += std::norm(cld(std::cos(wa * p), -std::sin(wa * p)) -
                                               cld(std::cos(wb * p), -std::sin(wb * p)));
    return std::sqrt(s);
}

// The FFT detector's bound (1) per ||x|| (fft_quad.hip, the shipped FUSED 4
// kernel). z = x_even + i x_odd (||z|| = ||x||), a 512-point
// complex FFT as a DFT-32 per lane (5 radix-2 levels: two plain, three fused
// t = fma(y, w.x, x), u = fma(y.yx, (-w.y, w.y), t), v = fma(x, 2, -u)) and
// a DFT-16 per column (4 fused levels, twiddles from fp32 tables), then the
// real post-pass. Every intermediate is a partial DFT of a decimated
// subsequence; at each level the nodes in a bin's cone partition z, so
// sum |node| <= sqrt(N) ||z|| (Cauchy-Schwarz). A plain level rounds once
// per component (|delta| <= u |out|); a fused level rounds t, u and (for the
// v output) v, each <= sqrt(L) ||z_node||, plus the fp32 twiddle's error
// |dw| <= u on |y| <= sqrt(L / 2) ||z_B||: (3 + 1 / sqrt 2) u sqrt(N) ||z||.
// X[k] = S / 2 + (W / 2) D, S = P + conj Q, D = -i (P - conj Q) carries the
// errors of Z[k] and Z[512 - k] with gain 1 each, plus the post-pass's own
// roundings (S, D, T = D W in two roundings, W's quantization, the final
// FMAs). The power moves sqrt P by u |X|, |X| <= sqrt(n) ||x||.
ld fft_rho(ld u)
{
    const ld N = 512.0L, rN = std::sqrt(N);
    const ld fused = 3.0L + 1.0L / std::sqrt(2.0L);
    const ld levels = 2.0L * 1.0L + 3.0L * fused + 4.0L * fused;  // DFT-32 + DFT-16
    const ld z = levels * u * rN;                                  // per-bin Z error
    const ld post = u * (3.0L * rN + 2.0L * rN + 32.0L);           // S/2, W dD, W quant; T; final
    const ld power = u * (32.0L + 2.0L * z + post);
    return (2.0L * z + post + power) * (1.0L + 1e-4L);             // (second order: < 1e-6 relative)
}

// The double radix-2 FFT oracle (oracle_fft_power) per bin, per ||x||: ten
// levels, each butterfly's t = w b with two products and a sum rounded per
// component, a +- t rounded, libm twiddles of a rounded angle (|dw| <= 10 u):
// <= 16 u sqrt(n) per level (generous); P = re^2 + im^2: u |X|.
ld fft_oracle_rho(int n)
{
    const ld rn = std::sqrt((ld)n);
    return (10.0L * 16.0L * kU64 * rn + kU64 * rn) * 1.01L;
}

// a lane's head: the 2-term rotation re = rx s1 - rz s2, im = ry s1 - rw s2
// over the core's outputs (s1, s2) = head inputs (0, 1)
LaneResult rot_lane(const Core &c, ld rx, ld ry, ld rz, ld rw, ld u)
{
    Lane H(2);
    int re, im;
    rotate2(H, 0, 1, rx, ry, rz, rw, re, im);
    return analyze_lane(c, H, re, im, u);
}

// fp32 bound (1) for one kernel slot, per sqrt(E_det)
ld detector_rho_slot(const demod_cfg_t &c, const Plan &pl, int sl)
{
    const int n = (int)c.n, G = 1 << pl.log2g;
    const int k = pl.slot_tone[sl];
    const ld u = kU32;
    if (pl.detector == kDetGoertzel) {
        // core: the 64-sample chain (plain or Reinsch form); head: segment j's rotation
        Lane L(64);
        std::vector<int> x(64);
        for (int i = 0; i < 64; ++i) x[i] = i;
        int s1, s2;
        if (pl.reinsch) chain_reinsch(L, x, pl.coef[sl], pl.sgn[sl], s1, s2);
        else chain_plain(L, x, pl.coef[sl], s1, s2);
        const Core core = analyze_core(L, {s1, s2});
        WindowAcc acc(n);
        std::vector<int> pos(64);
        for (int j = 0; j < G; ++j) {
            const float4 r = pl.rot[(size_t)sl * G + j];
            for (int i = 0; i < 64; ++i) pos[i] = 64 * j + i;
            acc.add(rot_lane(core, r.x, r.y, r.z, r.w, u), pos);
        }
        return acc.finish(std::acos((ld)pl.rcoef[k] / 2.0L), pl.log2g, u);
    }
    const ld wb = 2.0L * kPi * (ld)integer_bin(c, (uint32_t)k) / (ld)n;
    if (pl.detector == kDetFolded && pl.f16) {
        // lanes jj < 8 of the tone's half: xf[8 jj + i] and xf[64 + 8 jj + i],
        // combined exactly into Z0 (slots 0-3) or Z8 (slots 4-7)
        const ld sg = sl < 4 ? 1.0L : -1.0L;
        Lane L(16);
        std::vector<int> y(8);
        for (int i = 0; i < 8; ++i) y[i] = L.op({{i, 1.0L}, {8 + i, sg}}, false);
        int s1, s2;
        chain_plain(L, y, pl.coef[sl], s1, s2);
        const Core core = analyze_core(L, {s1, s2});
        WindowAcc acc(128);
        std::vector<int> pos(16);
        for (int jj = 0; jj < 8; ++jj) {
            const float4 r = pl.rot[(size_t)sl * 16 + jj];
            for (int i = 0; i < 8; ++i) {
                pos[i] = 8 * jj + i;
                pos[8 + i] = 64 + 8 * jj + i;
            }
            acc.add(rot_lane(core, r.x, r.y, r.z, r.w, u), pos);
        }
        return acc.finish(wb, 3, u);
    }
    if (pl.detector == kDetFolded) {
        Lane L(8);
        std::vector<int> y(8);
        for (int i = 0; i < 8; ++i) y[i] = i;
        int s1, s2;
        chain_plain(L, y, pl.coef[sl], s1, s2);
        const Core core = analyze_core(L, {s1, s2});
        WindowAcc acc(n / 8);
        std::vector<int> pos(8);
        for (int j = 0; j < G; ++j) {
            const float4 r = pl.rot[(size_t)sl * G + j];
            for (int i = 0; i < 8; ++i) pos[i] = 8 * j + i;
            acc.add(rot_lane(core, r.x, r.y, r.z, r.w, u), pos);
        }
        return acc.finish(wb, pl.log2g, u);
    }
    // residue: lane j's inputs are x[r + m P] (input m * 8 + i, r = 8 j + i);
    // core: the tone's class pair per folded position and its two chains
    const int P = n / 8;
    const ld kr = (ld)0.70710678118654752f;
    Lane L(64);
    std::vector<int> lo(8), hi(8);
    for (int i = 0; i < 8; ++i) {
        int x[8];
        for (int m = 0; m < 8; ++m) x[m] = 8 * m + i;
        const int a0 = L.op({{x[0], 1}, {x[4], 1}}, false), a2 = L.op({{x[2], 1}, {x[6], 1}}, false);
        const int d0 = L.op({{x[0], 1}, {x[4], -1}}, false), d2 = L.op({{x[2], 1}, {x[6], -1}}, false);
        const int a1 = L.op({{x[1], 1}, {x[5], 1}}, false), a3 = L.op({{x[3], 1}, {x[7], 1}}, false);
        const int d1 = L.op({{x[1], 1}, {x[5], -1}}, false), d3 = L.op({{x[3], 1}, {x[7], -1}}, false);
        switch (pl.zcls[sl]) {
        case 0: {  // (Z0, Z4)
            const int e0 = L.op({{a0, 1}, {a2, 1}}, false), e2 = L.op({{a1, 1}, {a3, 1}}, false);
            lo[i] = L.op({{e0, 1}, {e2, 1}}, false);
            hi[i] = L.op({{e0, 1}, {e2, -1}}, false);
            break;
        }
        case 3:  // (e1, e3)
            lo[i] = L.op({{a0, 1}, {a2, -1}}, false);
            hi[i] = L.op({{a1, 1}, {a3, -1}}, false);
            break;
        default: {  // Z1 = (d0 + kr u, -d2 - kr v), Z3 = (d0 - kr u, d2 - kr v)
            const int uu = L.op({{d1, 1}, {d3, -1}}, false), vv = L.op({{d1, 1}, {d3, 1}}, false);
            if (pl.zcls[sl] == 1) {
                lo[i] = L.op({{d0, 1}, {uu, kr}}, true);
                hi[i] = L.op({{d2, -1}, {vv, -kr}}, true);
            } else {
                lo[i] = L.op({{d0, 1}, {uu, -kr}}, true);
                hi[i] = L.op({{d2, 1}, {vv, -kr}}, true);
            }
        }
        }
    }
    int s1l, s2l, s1h, s2h;
    chain_plain(L, lo, pl.coef[sl], s1l, s2l);
    chain_plain(L, hi, pl.coef[sl], s1h, s2h);
    const Core core = analyze_core(L, {s1l, s1h, s2l, s2h});
    WindowAcc acc(n);
    std::vector<int> pos(64);
    for (int j = 0; j < G; ++j) {
        const float4 c12 = pl.rot[((size_t)sl * G + j) * 2], c34 = pl.rot[((size_t)sl * G + j) * 2 + 1];
        // X = c12.xy s1.lo; += c12.zw s1.hi; += c34.xy s2.lo; += c34.zw s2.hi (FMAs)
        Lane H(4);
        int re = H.op({{0, c12.x}}, true), im = H.op({{0, c12.y}}, true);
        re = H.op({{re, 1}, {1, c12.z}}, true);
        im = H.op({{im, 1}, {1, c12.w}}, true);
        re = H.op({{re, 1}, {2, c34.x}}, true);
        im = H.op({{im, 1}, {2, c34.y}}, true);
        re = H.op({{re, 1}, {3, c34.z}}, true);
        im = H.op({{im, 1}, {3, c34.w}}, true);
        for (int m = 0; m < 8; ++m)
            for (int i = 0; i < 8; ++i) pos[8 * m + i] = 8 * j + i + m * P;
        acc.add(analyze_lane(core, H, re, im, u), pos);
    }
    return acc.finish(wb, pl.log2g, u);
}

// pass 0 (double, n = 1024) for tone k at frequency w_ref with chain
// coefficient cc, per ||x||
ld first_pass_rho(const Plan &pl, uint32_t K, uint32_t k, ld w_ref)
{
    const double *r64 = pl.rot64.data();
    const ld cc = r64[(size_t)K * 64 + k];
    Lane L(64);
    std::vector<int> x(64);
    for (int i = 0; i < 64; ++i) x[i] = i;
    int s1, s2;
    chain_double(L, x, cc, s1, s2);
    const Core core = analyze_core(L, {s1, s2});
    WindowAcc acc(1024);
    std::vector<int> pos(64);
    for (int j = 0; j < 16; ++j) {
        const double *o = &r64[((size_t)k * 16 + j) * 4];
        for (int i = 0; i < 64; ++i) pos[i] = 64 * j + i;
        acc.add(rot_lane(core, o[0], o[1], o[2], o[3], kU64), pos);
    }
    return acc.finish(w_ref, 4, kU64);
}

// pass 0 by the fold (Plan::fold64) for tone k at its exact bin w_b, per
// ||xf|| (xf the window folded to 128 samples, exact; ||xf|| <= sqrt 8 ||x||):
// lane j's 8-step double chain over xf[8j .. 8j + 7], its rotation, the
// 16-lane tree, the power
ld first_pass_fold_rho(const Plan &pl, uint32_t K, uint32_t k, ld w_b)
{
    const double *r64 = pl.rot64.data();
    const ld cc = r64[(size_t)K * 64 + k];
    Lane L(8);
    std::vector<int> x(8);
    for (int i = 0; i < 8; ++i) x[i] = i;
    int s1, s2;
    chain_double(L, x, cc, s1, s2);
    const Core core = analyze_core(L, {s1, s2});
    WindowAcc acc(128);
    std::vector<int> pos(8);
    for (int j = 0; j < 16; ++j) {
        const double *o = &r64[((size_t)k * 16 + j) * 4];
        for (int i = 0; i < 8; ++i) pos[i] = 8 * j + i;
        acc.add(rot_lane(core, o[0], o[1], o[2], o[3], kU64), pos);
    }
    return acc.finish(w_b, 4, kU64);
}

// pass 0 by the residue fold (Plan::fold64 = 2) for tone k (bin b, residue
// rho = b mod 8) at w_b, per ||x||: lane j's 64 raw samples x[128 m + 8 j + i]
// (input 8 m + i), per position i the exact integer butterflies a_m = x_m +
// x_{m+4}, d_m = x_m - x_{m+4} (m < 4) and Y_rho = sum_m x_m e^{-2 pi i rho m
// / 8}: rho 0 / 4 real (a0 + a2 +- (a1 + a3)), rho 2 / 6 complex integers
// (a0 - a2, -+(a1 - a3)), odd rho d0 +- c u, -+d2 -+ c v with u = d1 - d3, v =
// d1 + d3, c = sqrt(2) / 2 in double (the products and sums rounded); two
// 8-step double chains (real and imaginary part; one for a real Y), the
// complex rotation X = A S1 - B S2 (every product and sum rounded), the
// 16-lane tree, the power (rescue.hip rescue_seg_kernel, op for op)
ld first_pass_residue_rho(const Plan &pl, uint32_t K, uint32_t k, ld w_b, int rho)
{
    const double *r64 = pl.rot64.data();
    const ld cc = r64[(size_t)K * 64 + k];
    const ld cq = (ld)0.70710678118654752440;  // (double) sqrt(2) / 2, as the kernel's constant
    Lane L(64);
    std::vector<int> yr(8), yi(8);
    const bool cplx = !(rho == 0 || rho == 4);
    for (int i = 0; i < 8; ++i) {
        int x[8];
        for (int m = 0; m < 8; ++m) x[m] = 8 * m + i;
        int a[4], d[4];
        for (int m = 0; m < 4; ++m) {
            a[m] = L.op({{x[m], 1}, {x[m + 4], 1}}, false);
            d[m] = L.op({{x[m], 1}, {x[m + 4], -1}}, false);
        }
        if (rho == 0 || rho == 4) {
            const ld sg = rho == 0 ? 1.0L : -1.0L;
            yr[i] = L.op({{a[0], 1}, {a[2], 1}, {a[1], sg}, {a[3], sg}}, false);
        } else if (rho == 2 || rho == 6) {
            yr[i] = L.op({{a[0], 1}, {a[2], -1}}, false);
            const ld sg = rho == 2 ? -1.0L : 1.0L;
            yi[i] = L.op({{a[1], sg}, {a[3], -sg}}, false);
        } else {
            const int u = L.op({{d[1], 1}, {d[3], -1}}, false), v = L.op({{d[1], 1}, {d[3], 1}}, false);
            const int cu = L.op({{u, cq}}, true), cv = L.op({{v, cq}}, true);
            const ld su = (rho == 1 || rho == 7) ? 1.0L : -1.0L;       // re = d0 +- c u
            const ld sd = (rho == 1 || rho == 5) ? -1.0L : 1.0L;       // im = +-d2 +- c v
            const ld sv = (rho == 1 || rho == 3) ? -1.0L : 1.0L;
            yr[i] = L.op({{d[0], 1}, {cu, su}}, true);
            yi[i] = L.op({{d[2], sd}, {cv, sv}}, true);
        }
    }
    int s1r, s2r, s1i = -1, s2i = -1;
    chain_double(L, yr, cc, s1r, s2r);
    if (cplx) chain_double(L, yi, cc, s1i, s2i);
    const Core core = cplx ? analyze_core(L, {s1r, s2r, s1i, s2i}) : analyze_core(L, {s1r, s2r});
    WindowAcc acc(1024);
    std::vector<int> pos(64);
    for (int j = 0; j < 16; ++j) {
        const double *o = &r64[((size_t)k * 16 + j) * 4];
        for (int m = 0; m < 8; ++m)
            for (int i = 0; i < 8; ++i) pos[8 * m + i] = 128 * m + 8 * j + i;
        if (!cplx) {
            acc.add(rot_lane(core, o[0], o[1], o[2], o[3], kU64), pos);
            continue;
        }
        // head over (S1r, S2r, S1i, S2i) = inputs 0 .. 3:
        // re = (Ar S1r - Ai S1i) - (Br S2r - Bi S2i), im = (Ar S1i + Ai S1r) - (Br S2i + Bi S2r)
        Lane H(4);
        const int p1 = H.op({{0, o[0]}}, true), p2 = H.op({{2, o[1]}}, true);
        const int t1 = H.op({{p1, 1}, {p2, -1}}, true);
        const int q1 = H.op({{1, o[2]}}, true), q2 = H.op({{3, o[3]}}, true);
        const int t2 = H.op({{q1, 1}, {q2, -1}}, true);
        const int re = H.op({{t1, 1}, {t2, -1}}, true);
        const int p3 = H.op({{2, o[0]}}, true), p4 = H.op({{0, o[1]}}, true);
        const int t3 = H.op({{p3, 1}, {p4, 1}}, true);
        const int q3 = H.op({{3, o[2]}}, true), q4 = H.op({{1, o[3]}}, true);
        const int t4 = H.op({{q3, 1}, {q4, 1}}, true);
        const int im = H.op({{t3, 1}, {t4, -1}}, true);
        acc.add(analyze_lane(core, H, re, im, kU64), pos);
    }
    return acc.finish(w_b, 4, kU64);
}

}  // namespace

void error_model(const demod_cfg_t &c, const Plan &pl, bool first_pass, ErrModel &m)
{
    m = ErrModel();
    const int n = (int)c.n;
    const bool fft = pl.detector == kDetFft, fold = pl.detector == kDetFolded;
    const bool bins = fft || fold || pl.detector == kDetResidue;
    // (2) the oracle, raw window
    ld ref = 0;
    for (uint32_t k = 0; k < c.k; ++k) {
        ld r;
        if (fft) {
            r = fft_oracle_rho(n);
        } else {
            r = oracle_rho(pl.rcoef[k], n);
            if (bins) {  // the detector evaluates the exact bin, the oracle its own frequency
                const ld wo = std::acos((ld)pl.rcoef[k] / 2.0L);
                const ld wb = 2.0L * kPi * (ld)integer_bin(c, k) / (ld)n;
                r += freq_gap(wo, wb, n);
            }
        }
        ref = std::max(ref, r);
    }
    // (1) the fp32 detector
    ld det = 0;
    if (fft) det = fft_rho(kU32);
    else
        for (uint32_t sl = 0; sl < c.k; ++sl) det = std::max(det, detector_rho_slot(c, pl, (int)sl));
    m.rho_det = (double)det;
    m.rho_ref = (double)ref;
    m.energy = fft ? DEMOD_ENERGY_PARSEVAL : fold ? DEMOD_ENERGY_FOLDED : DEMOD_ENERGY_RAW;
    // the flag test (plan.h): t2e E_eff >= 16 (bound)^2, with 1e-3 for the
    // fp32 evaluation of the test and of E (a sum of non-negative terms,
    // relative error < 100 u)
    const ld safe = (1.0L + 1e-3L) / (1.0L - 100.0L * kU32);
    const ld xmax2 = (ld)n * 1073741824.0L;  // int16: sum x^2 <= n 2^30
    ld t2e, emax, ne_per_e;
    if (fft) {
        // E = Parseval's 2 sum_{b<=512} P_b >= n sum x^2 (1 - 2e-4): the fp32
        // powers' norm-wise error is below rho_det sqrt(513) ||x|| against
        // ||X|| >= sqrt(n / 2) ||x||. (Tones-only batches whose tone bins
        // leave post-pass pair blocks unused skip those blocks and form E =
        // n sum x^2 from the samples instead: fft_quad.hip PICK 2, a 64-term
        // sum per lane and the 16-lane tree, within the 100 u above.)
        const ld rho = det + ref;
        t2e = 16.0L * rho * rho / (ld)n * safe / (1.0L - 2e-4L);
        emax = (ld)n * xmax2;
        ne_per_e = 1;
    } else if (fold) {
        const ld d = ref * std::sqrt(xmax2) / det;  // the oracle's share, in units of sqrt(E_f)
        m.amb_d = (double)d;
        t2e = 16.0L * det * det * safe;
        const ld ef = std::sqrt(8.0L * xmax2) + d;  // sum xf^2 <= 8 sum x^2
        emax = ef * ef;
        ne_per_e = n / 8.0L;
    } else {
        const ld rho = det + ref;
        t2e = 16.0L * rho * rho * safe;
        emax = xmax2;
        ne_per_e = n;
    }
    m.t2e = (double)t2e;
    m.tq = (double)(std::sqrt(t2e * emax) * (1.0L + 1e-3L));
    m.fl = (double)(t2e * emax / 16.0L);
    m.tau = (double)std::sqrt(t2e / ne_per_e);
    // pass 0 (n = 1024 in-kernel rescue; the FFT's tones-only batches): the
    // segmented double recurrence against the oracle, E its fp32 sum x^2
    if (first_pass && n == 1024 && c.k >= 2 && !pl.rot64.empty()) {
        ld f = 0;
        for (uint32_t k = 0; k < c.k; ++k) {
            ld r;
            if (pl.fold64) {
                // pass 0 evaluates the exact bin; the Goertzel oracle its own
                // frequency (the FFT oracle the bin)
                const long long b = fft ? pl.fft_bins[k] : integer_bin(c, k);
                const ld wb = 2.0L * kPi * (ld)b / (ld)n;
                r = pl.fold64 == 2 ? first_pass_residue_rho(pl, c.k, k, wb, (int)(b % 8))
                                   : std::sqrt(8.0L) * first_pass_fold_rho(pl, c.k, k, wb);
                if (fft) r += fft_oracle_rho(n);
                else r += freq_gap(std::acos((ld)pl.rcoef[k] / 2.0L), wb, n) + oracle_rho(pl.rcoef[k], n);
            } else {
                const ld w = fft ? 2.0L * kPi * (ld)pl.fft_bins[k] / 1024.0L
                                 : std::acos((ld)pl.rcoef[k] / 2.0L);
                r = first_pass_rho(pl, c.k, k, w) + (fft ? fft_oracle_rho(n) : oracle_rho(pl.rcoef[k], n));
            }
            f = std::max(f, r);
        }
        m.rho_first = (double)f;
        m.t2e64 = (double)(16.0L * f * f * safe);
        m.tau64 = (double)(4.0L * f / std::sqrt((ld)n));
    }
}

}  // namespace fskd

extern "C" int demod_error_model(const demod_cfg_t *cfg, demod_error_model_t *out)
{
    if (!cfg || !out) return DEMOD_BAD_ARG;
    const int rc = fskd::validate_cfg(cfg);
    if (rc != DEMOD_OK) return rc;
    fskd::Plan pl;
    fskd::build_plan(*cfg, pl);
    fskd::ErrModel m;
    fskd::error_model(*cfg, pl, true, m);
    std::memset(out, 0, sizeof(*out));
    out->method = pl.detector == fskd::kDetFolded    ? DEMOD_METHOD_FOLDED
                : pl.detector == fskd::kDetFft     ? DEMOD_METHOD_FFT
                : pl.detector == fskd::kDetResidue ? DEMOD_METHOD_RESIDUE
                                                   : DEMOD_METHOD_GOERTZEL;
    out->energy = m.energy;
    out->rho_det = m.rho_det;
    out->rho_ref = m.rho_ref;
    out->rho_first = m.rho_first;
    out->tau = cfg->k >= 2 ? m.tau : 0.0;
    out->tau64 = m.tau64;
    out->t2e = m.t2e;
    out->t2e64 = m.t2e64;
    out->amb_d = m.amb_d;
    return DEMOD_OK;
}

extern "C" int demod_plan_info(const demod_cfg_t *cfg, demod_plan_info_t *info, float *rot, size_t rot_cap,
                               double *rot64, size_t rot64_cap)
{
    if (!cfg || !info) return DEMOD_BAD_ARG;
    const int rc = fskd::validate_cfg(cfg);
    if (rc != DEMOD_OK) return rc;
    fskd::Plan pl;
    fskd::build_plan(*cfg, pl);
    std::memset(info, 0, sizeof(*info));
    info->method = pl.detector == fskd::kDetFolded    ? DEMOD_METHOD_FOLDED
                 : pl.detector == fskd::kDetFft     ? DEMOD_METHOD_FFT
                 : pl.detector == fskd::kDetResidue ? DEMOD_METHOD_RESIDUE
                                                    : DEMOD_METHOD_GOERTZEL;
    info->log2g = pl.log2g;
    info->reinsch = pl.reinsch;
    info->f16 = pl.f16;
    info->dcls = pl.dcls;
    info->slide = pl.slide;
    info->perm = pl.perm;
    for (int k = 0; k < fskd::kMaxTones; ++k) {
        info->slot_tone[k] = pl.slot_tone[k];
        info->zcls[k] = pl.zcls[k];
        info->fft_bins[k] = pl.fft_bins[k];
        info->coef[k] = pl.coef[k];
        info->sgn[k] = pl.sgn[k];
        info->rcoef[k] = pl.rcoef[k];
    }
    info->rot_len = (uint32_t)pl.rot.size();
    info->rot64_len = (uint32_t)pl.rot64.size();
    info->fold64 = pl.fold64;
    info->fft_pmask = pl.detector == fskd::kDetFft ? fskd::fft_quad_pmask(pl.fft_bins, (int)cfg->k) : 0u;
    if (rot && rot_cap >= 4 * pl.rot.size())
        std::memcpy(rot, pl.rot.data(), pl.rot.size() * sizeof(float4));
    if (rot64 && rot64_cap >= pl.rot64.size())
        std::memcpy(rot64, pl.rot64.data(), pl.rot64.size() * sizeof(double));
    return DEMOD_OK;
}
