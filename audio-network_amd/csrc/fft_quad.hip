// fft_quad.hip — the full-spectrum detector laid
// out as 16 lanes per window, 4 windows per wave: per window a 1024-point real
// FFT, |X[b]|^2 for b = 0..512, symbol = argmax over the tone bins (ties ->
// lowest k). Oracle: oracle/fsk_oracle.c:oracle_fft_demod.
//
// z[n] = x[2n] + i x[2n+1] (n < 512) is a 512-point complex FFT, split 32 x 16:
//   n = t + 16 n1 (t = lane % 16, n1 < 32),   k = k1 + 32 k2 (k1 < 32, k2 < 16)
//   Z[k1 + 32 k2] = sum_t W16^{t k2} W512^{t k1} sum_n1 z[t + 16 n1] W32^{n1 k1}
//   1. lane t loads its 32 dwords z[t + 16 n1] (16 lanes = 64 contiguous bytes
//      per instruction) and runs a DFT-32 in registers;
//   2. ONE transpose through LDS: row t -> columns. Lane t' takes the column
//      pair {k1, 32 - k1} (lane 0: {0, 16}) and runs, per column, the DFT-16
//      of the W512^{t k1}-twiddled column in registers;
//   3. the real-FFT post-pass pairs Z[k] with conj Z[512 - k]. With the column
//      pairing above that mirror lives in the same lane, so it needs no
//      exchange: per pair one twiddle product gives both |X[k]|^2 and
//      |X[512 - k]|^2.
// LDS traffic per window: 4 KiB written + 4 KiB read for the transpose (plus
// 2 KiB of bin powers when the full spectrum is stored) — against 12 + 12 KiB
// for a 64-lane radix-8 Stockham layout (scripts/fft_r0.hip, in git history
// at 8b49018), whose LDS writes
// bound it (guide: ds_write aggregates 38-51 TB/s). Every twiddle product is
// fused into the butterfly that consumes it (fft1024_quad_kernel below); the
// round-1 kernel with separate products is scripts/fft_quad_r1b.hip (git
// history, 8b49018).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "demod_internal.h"
#include "kernel_ops.h"
#include "rescue_fft.h"
#include "window_sum.h"

namespace fskd {
namespace quad {

// A complex number as a packed fp32 pair (lane_ops.h f2): complex add/sub is
// one v_pk_add_f32, a complex product two packed ops. CDNA4 runs a packed op at
// the same flop rate as two plain ones, but one wave issues half as many
// instructions — and this kernel is issue-bound (one wave/SIMD issues a VALU op
// every 4 cycles).

// lane % 16 == 0 ? a : b (lanes 0, 16, 32, 48 of the wave)
__device__ __forceinline__ f2 sel_l0(f2 a, f2 b)
{
    f2 r;
    // %0 %1 = r; %2 a.x, %3 b.x, %4 mask, %5 a.y, %6 b.y; dst = mask ? src1 : src0
    asm("v_cndmask_b32 %0, %3, %2, %4\n\tv_cndmask_b32 %1, %6, %5, %4"
        : "=&v"(r.x), "=v"(r.y)
        : "v"(a.x), "v"(b.x), "s"(0x0001000100010001ull), "v"(a.y), "v"(b.y));
    return r;
}

// W32^j = e^{-2 pi i j / 32}: real and imaginary parts.
constexpr float kW32r[32] = {
    1.0f, 0.98078528040323043f, 0.92387953251128674f, 0.83146961230254524f,
    0.70710678118654752f, 0.55557023301960218f, 0.38268343236508977f, 0.19509032201612827f,
    0.0f, -0.19509032201612827f, -0.38268343236508977f, -0.55557023301960218f,
    -0.70710678118654752f, -0.83146961230254524f, -0.92387953251128674f, -0.98078528040323043f,
    -1.0f, -0.98078528040323043f, -0.92387953251128674f, -0.83146961230254524f,
    -0.70710678118654752f, -0.55557023301960218f, -0.38268343236508977f, -0.19509032201612827f,
    0.0f, 0.19509032201612827f, 0.38268343236508977f, 0.55557023301960218f,
    0.70710678118654752f, 0.83146961230254524f, 0.92387953251128674f, 0.98078528040323043f};
constexpr float kW32i[32] = {
    0.0f, -0.19509032201612827f, -0.38268343236508977f, -0.55557023301960218f,
    -0.70710678118654752f, -0.83146961230254524f, -0.92387953251128674f, -0.98078528040323043f,
    -1.0f, -0.98078528040323043f, -0.92387953251128674f, -0.83146961230254524f,
    -0.70710678118654752f, -0.55557023301960218f, -0.38268343236508977f, -0.19509032201612827f,
    0.0f, 0.19509032201612827f, 0.38268343236508977f, 0.55557023301960218f,
    0.70710678118654752f, 0.83146961230254524f, 0.92387953251128674f, 0.98078528040323043f,
    1.0f, 0.98078528040323043f, 0.92387953251128674f, 0.83146961230254524f,
    0.70710678118654752f, 0.55557023301960218f, 0.38268343236508977f, 0.19509032201612827f};

template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// ---- fused twiddle butterflies (fft1024_quad_kernel) ----------------------
// A twiddled radix-2 butterfly (u, v) = (x + w y, x - w y) in three packed
// FMAs instead of a complex product (2) and two complex adds (2):
//   t = fma(y, w.xx, x)                    = (x.x + w.x y.x, x.y + w.x y.y)
//   u = fma(y.yx, (-w.y, w.y), t)          = x + w y
//   v = fma(x, 2, -u)                      = x - w y
// (v is 2x - u: one extra rounding of u, far inside the 1e-5 bar.) The -j w
// of a radix-4 butterfly's second output pair is the same register read with
// other op_sel / neg modifiers (-j w = (w.y, -w.x)), so it needs no table.
// Two independent pairs per asm block, interleaved so no packed result feeds
// the next instruction (gfx950 packed-fp32 write -> dependent read hazard).
#define QTB_T(U, Y, W, X) "v_pk_fma_f32 " U ", " Y ", " W ", " X " op_sel_hi:[1,0,1]\n\t"
#define QTB_U(U, Y, W) "v_pk_fma_f32 " U ", " Y ", " W ", " U " op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[0,1,0]\n\t"
#define QTB_TM(U, Y, W, X) "v_pk_fma_f32 " U ", " Y ", " W ", " X " op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
#define QTB_UM(U, Y, W) "v_pk_fma_f32 " U ", " Y ", " W ", " U " op_sel:[1,0,0] op_sel_hi:[0,0,1] neg_hi:[0,1,0]\n\t"
#define QTB_V(V, X, TWO, U) "v_pk_fma_f32 " V ", " X ", " TWO ", " U " neg_lo:[0,0,1] neg_hi:[0,0,1]"

// W32^E (a compile-time constant: an SGPR pair)
template <int E>
__device__ __forceinline__ f2 w32c()
{
    constexpr int j = ((E % 32) + 32) % 32;
    return (f2){kW32r[j], kW32i[j]};
}

// The geometric DFT-4: of (y0, w y1, w^2 y2, w^3 y3) at x[0], x[S], x[2S],
// x[3S] (natural order out), four fused butterflies in two stages,
//   a = y0 +- w^2 y2, c = y1 +- w^2 y3, X0/X2 = a0 +- w c0, X1/X3 = a1 +- (-j w) c1.
// Every form below is ONE asm block in which each result is read two or more
// instructions after it is written, so it needs none of the packed-write
// s_nops (and scheduling barriers) that separate blocks cost at their seams.
//
// Two independent geometric DFT-4s, each with a per-lane w (VGPRs) and its
// square w2, interleaved instruction by instruction (dependent results four
// instructions apart) and updated in place (the first stage's inputs are dead
// once it has run); the -j w pair by modifiers (QTB_TM / QTB_UM).
// %0-%3 / %4-%7 the two DFT-4s' x0..x3 (in / out), %8-%15 scratch a0 a1 c0 c1
// of each, %16 / %17 w / w^2 of the first, %18 / %19 of the second, %20 (2, 2).
template <int S>
__device__ __forceinline__ void dft4x2_fused_v(f2 *xa, f2 *xb, f2 wa, f2 w2a, f2 wb, f2 w2b)
{
    f2 a0, a1, c0, c1, b0, b1, d0, d1;
    asm(// first stage: a = x0 +- w^2 x2, c = x1 +- w^2 x3 (both DFT-4s)
        QTB_T("%8", "%2", "%17", "%0") QTB_T("%10", "%3", "%17", "%1")
        QTB_T("%12", "%6", "%19", "%4") QTB_T("%14", "%7", "%19", "%5")
        QTB_U("%8", "%2", "%17") QTB_U("%10", "%3", "%17")
        QTB_U("%12", "%6", "%19") QTB_U("%14", "%7", "%19")
        QTB_V("%9", "%0", "%20", "%8") "\n\t" QTB_V("%11", "%1", "%20", "%10") "\n\t"
        QTB_V("%13", "%4", "%20", "%12") "\n\t" QTB_V("%15", "%5", "%20", "%14") "\n\t"
        // second stage into x: X0/X2 = a0 +- w c0, X1/X3 = a1 +- (-j w) c1
        QTB_T("%0", "%10", "%16", "%8") QTB_TM("%1", "%11", "%16", "%9")
        QTB_T("%4", "%14", "%18", "%12") QTB_TM("%5", "%15", "%18", "%13")
        QTB_U("%0", "%10", "%16") QTB_UM("%1", "%11", "%16")
        QTB_U("%4", "%14", "%18") QTB_UM("%5", "%15", "%18")
        QTB_V("%2", "%8", "%20", "%0") "\n\t" QTB_V("%3", "%9", "%20", "%1") "\n\t"
        QTB_V("%6", "%12", "%20", "%4") "\n\t" QTB_V("%7", "%13", "%20", "%5")
        : "+v"(xa[0]), "+v"(xa[S]), "+v"(xa[2 * S]), "+v"(xa[3 * S]),
          "+v"(xb[0]), "+v"(xb[S]), "+v"(xb[2 * S]), "+v"(xb[3 * S]),
          "=&v"(a0), "=&v"(a1), "=&v"(c0), "=&v"(c1), "=&v"(b0), "=&v"(b1), "=&v"(d0), "=&v"(d1)
        : "v"(wa), "v"(w2a), "v"(wb), "v"(w2b), "s"((f2){2.0f, 2.0f}));
}

// The geometric DFT-4 with w = W32^E when neither w^2 = W32^{2E} nor w is a
// quarter turn: first stage both pairs with w^2, second stage w and -j w =
// W32^{E+8}, all SGPR constants (%12 w, %13 w^2, %15 -j w).
#define QF_STAGES_K                                                                         \
    QTB_T("%4", "%10", "%13", "%8") QTB_T("%6", "%11", "%13", "%9")                        \
    QTB_U("%4", "%10", "%13") QTB_U("%6", "%11", "%13")                                    \
    QTB_V("%5", "%8", "%14", "%4") "\n\t" QTB_V("%7", "%9", "%14", "%6") "\n\t"         \
    QTB_T("%0", "%6", "%12", "%4") QTB_T("%1", "%7", "%15", "%5")                           \
    QTB_U("%0", "%6", "%12") QTB_U("%1", "%7", "%15")                                       \
    QTB_V("%2", "%4", "%14", "%0") "\n\t" QTB_V("%3", "%5", "%14", "%1")
template <int E, int S>
__device__ __forceinline__ void dft4_fused_k(f2 *x)
{
    f2 X0, X1, X2, X3, a0, a1, c0, c1;
    asm(QF_STAGES_K
        : "=&v"(X0), "=&v"(X1), "=&v"(X2), "=&v"(X3), "=&v"(a0), "=&v"(a1), "=&v"(c0), "=&v"(c1)
        : "v"(x[0]), "v"(x[S]), "v"(x[2 * S]), "v"(x[3 * S]), "s"(w32c<E>()), "s"(w32c<2 * E>()),
          "s"((f2){2.0f, 2.0f}), "s"(w32c<E + 8>()));
    x[0] = X0;
    x[S] = X1;
    x[2 * S] = X2;
    x[3 * S] = X3;
}

// The trivial-twiddle pieces of the DFT-32 as single blocks too.
// x + (-j) y and x - (-j) y as instruction text
#define QA_MJ(R, X, Y) "v_pk_add_f32 " R ", " X ", " Y " op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]\n\t"
#define QS_MJ(R, X, Y) "v_pk_add_f32 " R ", " X ", " Y " op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]\n\t"
#define QADD(R, X, Y) "v_pk_add_f32 " R ", " X ", " Y "\n\t"
#define QSUB(R, X, Y) "v_pk_add_f32 " R ", " X ", " Y " neg_lo:[0,1] neg_hi:[0,1]\n\t"
// DFT-4 with no twiddles (w = 1): 8 packed adds.
// %0-%3 X0..X3, %4-%7 a0 a1 c0 c1, %8-%11 x0..x3
template <int S>
__device__ __forceinline__ void dft4_triv(f2 *x)
{
    f2 X0, X1, X2, X3, a0, a1, c0, c1;
    asm(QADD("%4", "%8", "%10") QSUB("%5", "%8", "%10") QADD("%6", "%9", "%11") QSUB("%7", "%9", "%11")
        QADD("%0", "%4", "%6") QSUB("%2", "%4", "%6") QA_MJ("%1", "%5", "%7")
        "v_pk_add_f32 %3, %5, %7 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]"
        : "=&v"(X0), "=&v"(X1), "=&v"(X2), "=&v"(X3), "=&v"(a0), "=&v"(a1), "=&v"(c0), "=&v"(c1)
        : "v"(x[0]), "v"(x[S]), "v"(x[2 * S]), "v"(x[3 * S]));
    x[0] = X0;
    x[S] = X1;
    x[2 * S] = X2;
    x[3 * S] = X3;
}
// The geometric DFT-4 with w^2 = -j (E = 4): first stage QA_MJ / QS_MJ, second
// stage w = W32^E and -j w = W32^{E+8} (%12, %13 SGPR pairs, %14 (2, 2)).
template <int E, int S>
__device__ __forceinline__ void dft4_fused_kq(f2 *x)
{
    static_assert(((2 * E) % 32 + 32) % 32 == 8, "w^2 = -j");
    f2 X0, X1, X2, X3, a0, a1, c0, c1;
    asm(QA_MJ("%4", "%8", "%10") QA_MJ("%6", "%9", "%11") QS_MJ("%5", "%8", "%10") QS_MJ("%7", "%9", "%11")
        QTB_T("%0", "%6", "%12", "%4") QTB_T("%1", "%7", "%13", "%5")
        QTB_U("%0", "%6", "%12") QTB_U("%1", "%7", "%13")
        QTB_V("%2", "%4", "%14", "%0") "\n\t" QTB_V("%3", "%5", "%14", "%1")
        : "=&v"(X0), "=&v"(X1), "=&v"(X2), "=&v"(X3), "=&v"(a0), "=&v"(a1), "=&v"(c0), "=&v"(c1)
        : "v"(x[0]), "v"(x[S]), "v"(x[2 * S]), "v"(x[3 * S]), "s"(w32c<E>()), "s"(w32c<E + 8>()),
          "s"((f2){2.0f, 2.0f}));
    x[0] = X0;
    x[S] = X1;
    x[2 * S] = X2;
    x[3 * S] = X3;
}
// The DFT-8's last stage (dftf<8>): pairs (slot 2k1, 2k1 + 1) with W8^k1:
// k1 = 0 trivial, 2 is -j, 1 and 3 general (W32^4, W32^12), interleaved.
// %0-%7 out slots 0..7 (u0 u1 u2 u3 v0 v1 v2 v3), %8-%15 in, %16 W32^4,
// %17 W32^12, %18 (2, 2)
template <int S>
__device__ __forceinline__ void dft8_last(f2 *x)
{
    f2 u0, u1, u2, u3, v0, v1, v2, v3;
    asm(QTB_T("%1", "%11", "%16", "%10") QTB_T("%3", "%15", "%17", "%14")
        QADD("%0", "%8", "%9") QSUB("%4", "%8", "%9")
        QTB_U("%1", "%11", "%16") QTB_U("%3", "%15", "%17")
        QA_MJ("%2", "%12", "%13") QS_MJ("%6", "%12", "%13")
        QTB_V("%5", "%10", "%18", "%1") "\n\t" QTB_V("%7", "%14", "%18", "%3")
        : "=&v"(u0), "=&v"(u1), "=&v"(u2), "=&v"(u3), "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
        : "v"(x[0]), "v"(x[S]), "v"(x[2 * S]), "v"(x[3 * S]), "v"(x[4 * S]), "v"(x[5 * S]),
          "v"(x[6 * S]), "v"(x[7 * S]), "s"(w32c<4>()), "s"(w32c<12>()), "s"((f2){2.0f, 2.0f}));
    x[0] = u0; x[S] = u1; x[2 * S] = u2; x[3 * S] = u3;
    x[4 * S] = v0; x[5 * S] = v1; x[6 * S] = v2; x[7 * S] = v3;
}

// In-register DFT of x[0], x[S], .., x[(N-1) S] (N = 4, 8, 16, 32), natural
// order out, every twiddle fused into the butterfly that consumes it.
// Mixed radix N = N1 x N2 (N2 = 4, or 2 at N = 8): DFT-N1 over i1 for each i2,
// then per k1 a DFT-N2 over i2 of the twiddled column, which is geometric in
// w = W_N^{k1}: the asm block written for its twiddles (w = 1: dft4_triv;
// w^2 = -j: dft4_fused_kq; else dft4_fused_k; the DFT-8's last stage:
// dft8_last).
template <int N, int S = 1>
__device__ __forceinline__ void dftf(f2 *x)
{
    if constexpr (N == 4) {
        dft4_triv<S>(x);
    } else if constexpr (N == 8) {
        dftf<4, 2 * S>(x);       // i2 = 0: X[k1] at slot 2 k1
        dftf<4, 2 * S>(x + S);   // i2 = 1: X[k1] at slot 2 k1 + 1
        // per k1: (slot 2k1, slot 2k1+1) -> X[k1], X[k1 + 4], twiddle W8^k1 = W32^{4 k1}
        dft8_last<S>(x);
    } else {
        constexpr int N1 = N / 4;   // 8 (N = 32) or 4 (N = 16)
        static_for<0, 4>([&](auto c) {
            constexpr int i2 = decltype(c)::value;
            dftf<N1, 4 * S>(x + i2 * S);   // X[k1] of column i2 at slot i2 + 4 k1
        });
        static_for<0, N1>([&](auto d) {
            constexpr int k1 = decltype(d)::value;
            constexpr int E = k1 * (32 / N);
            static_assert(E >= 0 && E < 8, "w = W32^E short of a quarter turn");
            if constexpr (E == 0)
                dft4_triv<S>(x + 4 * k1 * S);
            else if constexpr (E == 4)
                dft4_fused_kq<E, S>(x + 4 * k1 * S);
            else
                dft4_fused_k<E, S>(x + 4 * k1 * S);   // slot 4 k1 + k2 = X[k1 + N1 k2]
        });
        f2 t[N];
        static_for<0, N>([&](auto e) {
            constexpr int m = decltype(e)::value;  // m = 4 k1 + k2
            t[(m / 4) + N1 * (m % 4)] = x[m * S];
        });
        static_for<0, N>([&](auto e) {
            constexpr int m = decltype(e)::value;
            x[m * S] = t[m];
        });
    }
}

// Two mirror pairs of the real post-pass as one block (16 packed ops):
// S = P + conj Q, D = -i (P - conj Q), T = D (W / 2), (re, im) of X[kP] and
// X[512 - kP] side by side, powers (|X[kP]|^2, |X[512 - kP]|^2). Interleaved
// so every result is read two instructions after it is written.
// Operands: %0 %1 pw0 pw1 (out), %2-%9 scratch S0 S1 D0 D1 T0 T1 R0 R1,
// %10 P0, %11 Q0, %12 W0, %13 P1, %14 Q1, %15 W1, %16 (1/2, 1/2).
__device__ __forceinline__ void postpair2(f2 &pw0, f2 P0, f2 Q0, f2 W0, f2 &pw1, f2 P1, f2 Q1, f2 W1)
{
    f2 S0, S1, D0, D1, T0, T1, R0, R1;
    asm("v_pk_add_f32 %2, %10, %11 neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %3, %13, %14 neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %4, %10, %11 op_sel:[1,1] op_sel_hi:[0,0] neg_hi:[1,0]\n\t"
        "v_pk_add_f32 %5, %13, %14 op_sel:[1,1] op_sel_hi:[0,0] neg_hi:[1,0]\n\t"
        "v_pk_mul_f32 %6, %4, %12 op_sel:[1,1] op_sel_hi:[1,0]\n\t"
        "v_pk_mul_f32 %7, %5, %15 op_sel:[1,1] op_sel_hi:[1,0]\n\t"
        "v_pk_fma_f32 %6, %4, %12, %6 op_sel_hi:[0,1,1] neg_lo:[0,0,1]\n\t"
        "v_pk_fma_f32 %7, %5, %15, %7 op_sel_hi:[0,1,1] neg_lo:[0,0,1]\n\t"
        "v_pk_fma_f32 %8, %2, %16, %6 op_sel_hi:[0,1,0] neg_hi:[0,0,1]\n\t"
        "v_pk_fma_f32 %9, %3, %16, %7 op_sel_hi:[0,1,0] neg_hi:[0,0,1]\n\t"
        "v_pk_fma_f32 %4, %2, %16, %6 op_sel:[1,0,1] neg_hi:[0,0,1]\n\t"
        "v_pk_fma_f32 %5, %3, %16, %7 op_sel:[1,0,1] neg_hi:[0,0,1]\n\t"
        "v_pk_mul_f32 %6, %4, %4\n\t"
        "v_pk_mul_f32 %7, %5, %5\n\t"
        "v_pk_fma_f32 %0, %8, %8, %6\n\t"
        "v_pk_fma_f32 %1, %9, %9, %7"
        : "=&v"(pw0), "=&v"(pw1), "=&v"(S0), "=&v"(S1), "=&v"(D0), "=&v"(D1), "=&v"(T0), "=&v"(T1),
          "=&v"(R0), "=&v"(R1)
        : "v"(P0), "v"(Q0), "v"(W0), "v"(P1), "v"(Q1), "v"(W1), "s"((f2){0.5f, 0.5f}));
}

}  // namespace quad

// Per-wave LDS: 4 windows x 16 rows x 17 complex (8704 B). The transpose
// moves half the columns per round (k1 < 16, then k1 >= 16), so only half of
// the DFT-32 output and half of the DFT-16 input are live at once. Row stride
// 34 words: the 16 lanes of a row write (ds_write_b64) cover 32 banks; the
// window stride 544 words = 32 mod 64 puts odd windows on the other 32, so a
// 32-lane pass of writes or column reads is conflict-free. Reused for the bin
// powers (4 x 513 floats).
// Bin powers after step 3, per window (stride kQPow floats): pair j of lane t
// stores (|X[kP]|^2, |X[512 - kP]|^2) as one f2 at slot 16 j + t; lane 0's
// |X[0]|^2, |X[512]|^2 sit at floats 512, 513. quad_slot(b) is the float
// index of bin b.
constexpr int kQPow = 544;  // floats per window: 8-byte aligned, odd windows on the other 32 banks
__host__ __device__ constexpr int quad_slot(int b)
{
    const int u = b & 31, v = b >> 5;
    // lane 0: pairs j < 8 hold kP = 16 + 32 j, pair 8 |X[256]|^2 twice,
    // pairs j > 8 kP = 32 j; |X[0]|^2 and |X[512]|^2 at floats 512, 513
    if (b == 0 || b == 512) return 512 + (b >> 9);
    if (u == 0) return v > 8 ? 2 * (16 * v) : v == 8 ? 256 : 2 * (16 * (16 - v)) + 1;
    if (u == 16) return v < 8 ? 2 * (16 * v) : 2 * (16 * (15 - v)) + 1;
    if (u < 16) return 2 * (16 * v + u);                 // kP = t + 32 j
    return 2 * (16 * (15 - v) + (32 - u)) + 1;           // mirror 512 - kP
}

constexpr int kQRow = 17;            // complex per row (16 + 1 pad)
constexpr int kQWin = 16 * kQRow;    // complex per window
constexpr int kQSlab = 4 * kQWin;    // complex per wave
static_assert(4 * kQPow <= 2 * kQSlab, "bin powers of 4 windows must fit the slab");

// fft1024_quad_kernel (round 2): the quad layout with every twiddle fused into the
// butterfly that consumes it (dftf, dft4x2_fused_v), the stage-1 twiddle moved
// behind the transpose and the 1/2 of the real split folded into the
// post-pass FMAs:
//   * stage 1: DFT-32 over n1 (compile-time twiddles fused), transposed raw;
//   * stage 2: lane t' runs, per column col in {t', k1b}, the DFT-16 over rows
//     t of A_t[col] W512^{t col}. With t = i2 + 4 i1 the twiddle factors as
//     W512^{i2 col} W128^{i1 col}: the inner DFT-4 over i1 is geometric in
//     v = W128^col, and W512^{i2 col} moves onto its outputs, where it joins
//     W16^{i2 k1} into the outer DFT-4's ratio g_k1 = W512^{col + 32 k1}; per
//     lane and column v, v^2, g_k1, g_k1^2 come from a 2.5 KiB LDS table
//     (tw2), -j w by operand modifiers;
//   * post-pass: T = (W/2) D (tw3 holds W1024^kP / 2), (re, im) pairs by FMA
//     with 1/2 (postpair2).
// 514 instead of 575 packed instructions per group of 4 windows.
// 4-wave blocks, 4 waves per SIMD asked for (104-116 VGPRs without spills);
// each group loads at the top of its iteration and the co-resident waves
// cover the latency; every DFT-4 stage pair, the DFT-32's trivial pieces and
// the post-pass pairs are single asm blocks (stage 2: two DFT-4s per block).
// SPEC: false = symbols (+ tone powers) only: the tone powers are picked
// from the registers of the lanes that hold them (p.slot, a wave-uniform
// index: s_set_gpr_idx) instead of going through the 2 KiB per-window power
// slab in LDS; true = the slab, for the full-spectrum store.
// PICK (SPEC false; 0 with SPEC): 1 = tone i's power is gathered into lane i
// of its row by one ds_bpermute, so lanes t < K hold tone t like the slab pick
// leaves them (4 VALU per tone, one coalesced magnitude store); 2 = the same
// over only the post-pass pair blocks that hold a tone bin (p.pmask).
// AUX: the loads' cache-policy bits (2 = nt, 0 = plain; launch_fft_quad).
// SPL (with SPEC): 2 = the bin powers go to the slab as the output's own
// layout (4 windows x 513 floats, contiguous, bin b of window q at float
// 513 q + b; each lane's pair j lands at its bins by immediate offsets), and
// the group's live windows leave as one contiguous run of non-temporal
// 16-byte stores (9 ds_read_b128 + 9 dwordx4 stores per lane, 1 KiB per wave
// instruction; the spectrum is written once);
// 0 = the quad_slot layout, 33 scattered dword stores per lane.
// OVL: round 1 of the transpose overlaps column 0's DFT-16. Column
// 0's twiddles are read right behind round 0's column reads, round 1's writes
// and reads follow, and column 0's DFT-16 runs while they are in flight (the
// waits land on the first use of round 1's data, not before column 0's
// math); the next group's round-0 writes are ordered behind them.
// Variants scripts/fft_probe.hip tried and did not ship; their source is in
// git history at f48c2d8 (the measurements: DESIGN.md §4.4):
//   PF 1 / 2   the next group's 32 loads during the transpose, or after the
//              post-pass ahead of the spectrum stores: 1.71-1.94 ms against
//              1.71 ms at hop 256 with 3 or 4 waves per SIMD.
//   WPB, MINW  other block sizes and waves-per-SIMD requests (as above).
//   FMT        typed buffer loads (16_16 SSCALED) convert both int16 halves
//              in the texture path, 64 VALU converts fewer per group: +-2 %.
//   FUSED < 4  fewer pieces as single asm blocks (the separate blocks cost an
//              s_nop and a scheduling barrier at every seam): launch_fft_quad
//              has the numbers.
//   RD 1 / 2   (fft1024_quad_kernel_r64) the backend's LDS-access pairing off,
//              and the twiddle tables lane-major, one ds_read_b128 per pair:
//              1.699 / 1.660 ms against 1.661 ms.
//   SPL 1      the linear slab with plain stores: 2.85-2.89 ms against 2.73 ms
//              non-temporal.
//   TW3R       the post-pass twiddles W1024^kP / 2 from registers (a per-lane
//              base times the compile-time W32^j) instead of the LDS table
//              tw3: -1 %, but other bits than the table's.
//   RSC 0 / 2  no in-kernel rescue (probe A/B), and the block's flagged
//              windows dealt round-robin to its waves.
//   PICK 0     without SPEC: each lane keeps the best and second tone it owns
//              (~27 VALU per tone), then the row argmax: +1.7 to 1.8 %.
template <bool SPEC, int AUX, int SPL, int OVL, int PICK>
__device__ __attribute__((always_inline)) inline void fft1024_quad_body(const FftParams &p)
{
    constexpr int WPB = 4;
    static_assert(SPL == 0 || (SPEC && SPL == 2), "SPL: the linear power slab of the spectrum store");
    static_assert(SPEC ? PICK == 0 && !OVL : PICK == 1 || PICK == 2, "PICK: the tones-only tone pick");
    using namespace quad;
    __shared__ __attribute__((aligned(16))) f2 slab[WPB][kQSlab];
    // tw2 [column slot][v, v2, g0, g0^2, .., g3, g3^2][t], tw3 [j][t]
    __shared__ __attribute__((aligned(16))) f2 tw2[2 * 10 * 16];
    __shared__ __attribute__((aligned(16))) f2 tw3[16 * 16];
    auto tw2_at = [](int sl, int m, int tt) { return sl * 160 + m * 16 + tt; };
    auto tw3_at = [](int j, int tt) { return j * 16 + tt; };
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane >> 4;   // window of the wave
    const int t = lane & 15;   // row / column-pair index
    const f2 *t512 = reinterpret_cast<const f2 *>(p.tw512);
    const f2 *t1024 = reinterpret_cast<const f2 *>(p.tw1024);
    for (int i = threadIdx.x; i < 2 * 10 * 16; i += 64 * WPB) {
        const int tt = i & 15, m = (i >> 4) % 10, sl = i / 160;
        const int col = sl == 0 ? tt : (tt == 0 ? 16 : 32 - tt);
        int e;  // exponent of W512
        if (m == 0) e = 4 * col;                          // v = W128^col
        else if (m == 1) e = 8 * col;                     // v^2
        else {
            const int k1 = (m - 2) >> 1;
            e = (col + 32 * k1) * (((m - 2) & 1) ? 2 : 1);   // g_k1, g_k1^2
        }
        tw2[tw2_at(sl, m, tt)] = t512[e & 511];
    }
    for (int i = threadIdx.x; i < 16 * 16; i += 64 * WPB) {
        const int tt = i & 15, j = i >> 4;
        tw3[tw3_at(j, tt)] = 0.5f * t1024[(tt == 0 && j < 8) ? 16 + 32 * j : tt + 32 * j];
    }
    const int k1b = t == 0 ? 16 : 32 - t;
    const int mybin = t < p.k ? p.bins[t] : 0;
    const int myslot = SPL ? q * 513 + mybin : quad_slot(mybin);
    float *pw = reinterpret_cast<float *>(slab[wave]);
    const int rowaddr = (lane & 48) * 4;  // byte address of this window row's lane 0 (ds_bpermute)
    __syncthreads();

    const long long n_groups = (p.n_windows + 3) >> 2;
    const long long stride = (long long)gridDim.x * WPB;
    long long g = tile_block(p.xcd_swizzle) * WPB + wave;
    const long long g_first = g;
    uint32_t nx[32];
    // One buffer descriptor per group (wave-uniform base = its first window);
    // the lane offset is the window's start + 4 t bytes, and z[t + 16 n1] is
    // the immediate offset 64 n1 (< 4 KiB). Windows past the end are clamped
    // to the last (never stored).
    auto load_group = [&](long long gg) {
        const long long w0 = 4 * gg;
        const long long left = p.n_windows - w0;  // >= 1
        const long long wq = q < left ? q : left - 1;
        // (lane_ops.h tile_rsrc, spelled out: through it the compiler orders
        // the kernel's scalar loads differently)
        long long bytes = ((left - 1) * p.hop + 1024) * 2;
        if (bytes > 0x7FFFFFF0LL) bytes = 0x7FFFFFF0LL;
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(p.pcm + w0 * p.hop), (short)0, (int)bytes, 0x00020000);
        const int voff = (int)(wq * p.hop * 2) + 4 * t;
#pragma unroll
        for (int n1 = 0; n1 < 32; ++n1)
            nx[n1] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff + 64 * n1, 0, AUX);
    };
    for (; g < n_groups; g += stride) {
        const long long w = 4 * g + q;
        load_group(g);
        f2 a[32];
#pragma unroll
        for (int n1 = 0; n1 < 32; ++n1) {
            a[n1] = (f2){(float)(int)(short)(nx[n1] & 0xFFFFu), (float)((int)nx[n1] >> 16)};
            asm("" : "+v"(a[n1]));  // opaque: keep (float)a + (float)b a packed add
        }

        // 1. DFT-32 over n1 (fused twiddles), no stage-1 twiddle here
        dftf<32>(a);

        // 2. transpose in two column rounds; lane (q, t') gets columns
        //    k1 = t' (round 0) and k1b (round 1) of its window
        f2 b[32];  // b[n2] = A_n2[t'], b[16 + n2] = A_n2[k1b]
        f2 *win = slab[wave] + q * kQWin;
        // twp(sl, m): the pair (m, m + 1) of slot sl, m even
        auto twp = [&](int sl, int m, f2 &lo, f2 &hi) {
            lo = tw2[tw2_at(sl, m, t)];
            hi = tw2[tw2_at(sl, m + 1, t)];
        };
        // natural order of one column's DFT-16 outputs
        auto col16_order = [&](f2 *bb) {
            f2 tt[16];
            static_for<0, 16>([&](auto e) {
                constexpr int m = decltype(e)::value;  // m = 4 k1 + k2 holds Z[col + 32 (k1 + 4 k2)]
                tt[(m / 4) + 4 * (m % 4)] = bb[m];
            });
            static_for<0, 16>([&](auto e) {
                constexpr int m = decltype(e)::value;
                bb[m] = tt[m];
            });
        };
        if constexpr (OVL) {
            // one column's DFT-16 with its ten twiddles given
            auto col16 = [&](f2 *bb, f2 v, f2 v2, f2 g0, f2 g0s, f2 g1, f2 g1s, f2 g2, f2 g2s, f2 g3,
                             f2 g3s) {
                dft4x2_fused_v<4>(bb + 0, bb + 1, v, v2, v, v2);
                dft4x2_fused_v<4>(bb + 2, bb + 3, v, v2, v, v2);
                dft4x2_fused_v<1>(bb + 0, bb + 4, g0, g0s, g1, g1s);
                dft4x2_fused_v<1>(bb + 8, bb + 12, g2, g2s, g3, g3s);
                col16_order(bb);
            };
            // the previous group's round-1 reads stay ahead of these writes
            // (LDS executes one wave's operations in order)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int c = 0; c < 16; ++c) win[t * kQRow + c] = a[c];
            wave_sync();
#pragma unroll
            for (int n2 = 0; n2 < 16; ++n2) b[n2] = win[n2 * kQRow + t];
            f2 v, v2, g0, g0s, g1, g1s, g2, g2s, g3, g3s;
            twp(0, 0, v, v2);
            twp(0, 2, g0, g0s);
            twp(0, 4, g1, g1s);
            twp(0, 6, g2, g2s);
            twp(0, 8, g3, g3s);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int c = 0; c < 16; ++c) win[t * kQRow + c] = a[16 + c];
            wave_sync();
#pragma unroll
            for (int n2 = 0; n2 < 16; ++n2) b[16 + n2] = win[n2 * kQRow + k1b - 16];
            col16(b, v, v2, g0, g0s, g1, g1s, g2, g2s, g3, g3s);
            twp(1, 0, v, v2);
            twp(1, 2, g0, g0s);
            twp(1, 4, g1, g1s);
            twp(1, 6, g2, g2s);
            twp(1, 8, g3, g3s);
            col16(b + 16, v, v2, g0, g0s, g1, g1s, g2, g2s, g3, g3s);
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int c = 0; c < 16; ++c) win[t * kQRow + c] = a[16 * r + c];
                wave_sync();
                const int col = r == 0 ? t : k1b - 16;
#pragma unroll
                for (int n2 = 0; n2 < 16; ++n2) b[16 * r + n2] = win[n2 * kQRow + col];
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            // 3. per column: DFT-16 over t of A_t[col] W512^{t col}, twiddles fused
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                f2 *bb = b + 16 * sl;
                f2 v, v2;
                twp(sl, 0, v, v2);
                dft4x2_fused_v<4>(bb + 0, bb + 1, v, v2, v, v2);
                dft4x2_fused_v<4>(bb + 2, bb + 3, v, v2, v, v2);
                f2 g0, g0s, g1, g1s, g2, g2s, g3, g3s;
                twp(sl, 2, g0, g0s);
                twp(sl, 4, g1, g1s);
                twp(sl, 6, g2, g2s);
                twp(sl, 8, g3, g3s);
                dft4x2_fused_v<1>(bb + 0, bb + 4, g0, g0s, g1, g1s);
                dft4x2_fused_v<1>(bb + 8, bb + 12, g2, g2s, g3, g3s);
                col16_order(bb);
            }
        }
        // b[k2] = Z[t + 32 k2], b[16 + k2] = Z[k1b + 32 k2] (unscaled)

        // 4. real post-pass over 16 mirror pairs, as fft1024_quad_kernel step 3
        //    with X[kP] = S/2 + (W/2) D and the powers of both mirrors per pair
        const bool l0 = (t == 0);
        float *pq = pw + q * kQPow;
        // SPL: float index of (|X[kP]|^2, |X[512 - kP]|^2) of pair j, as row
        // base + 32 j and mirror base + 32 (15 - j): lane t has kP = t + 32 j;
        // lane 0 has kP = 16 + 32 j for j < 8 (like t = 16) and 32 j for
        // j >= 8. Formed here from the lane id, fenced from hoisting, so the
        // four bases do not stay live across the group loop (with them the
        // kernel hit 128 VGPRs and spilled 20 B per lane).
        int tl = (int)(threadIdx.x & 63);
        if constexpr (SPL) asm volatile("" : "+v"(tl));
        const int tt = tl & 15, rowb = (tl >> 4) * 513;
        const int te_lo = tt == 0 ? 16 : tt;
        const int spl_a_lo = rowb + te_lo, spl_m_lo = rowb + 32 - te_lo;
        const int spl_a_hi = rowb + tt, spl_m_hi = rowb + 32 - tt;
        f2 *const ps = reinterpret_cast<f2 *>(pq) + t;  // slot (j, t) at ps[16 j]
        // !SPEC: this lane's powers, pv[2 j + half], one 32-register tuple so a
        // uniform index reads it with v_movrels (no scratch, no select chain)
        typedef float f32x32 __attribute__((ext_vector_type(32)));
        f32x32 pv;
        static_for<0, 8>([&](auto jc) {
            constexpr int j0 = 2 * decltype(jc)::value, j1 = j0 + 1;
            f2 pw0, pw1;  // (|X[kP]|^2, |X[512-kP]|^2)
            // PICK 2: only the pair blocks holding a tone bin (p.pmask,
            // wave-uniform: a scalar branch per block; the skipped blocks'
            // powers are undefined and never read, and only their values,
            // not the power tuple, merge at the branch). The empty asm
            // defines them without an instruction (left undefined, the
            // compiler zeroed them: 4 v_mov per block, executed or not)
            if constexpr (!SPEC && PICK == 2) asm volatile("" : "=v"(pw0), "=v"(pw1));
            const bool need = SPEC || PICK != 2 || ((p.pmask >> decltype(jc)::value) & 1u);
            if (need) {
            f2 P0 = b[j0], Q0 = b[16 + 15 - j0];
            f2 P1 = b[j1], Q1 = b[16 + 15 - j1];
            // lane 0 (columns 0 and 16): pairs j < 8 are column 16's
            // (Z[16 + 32 j], mirror in the default Q slot), pairs j >= 8
            // column 0's (Z[32 j] with Z[32 (16 - j)]; j = 8 is Z[256] with
            // itself): 16 selects instead of 24 for the layout before
            if constexpr (j0 < 8) {
                P0 = sel_l0(b[16 + j0], P0);
                P1 = sel_l0(b[16 + j1], P1);
            } else {
                Q0 = sel_l0(b[16 - j0], Q0);
                Q1 = sel_l0(b[16 - j1], Q1);
            }
            const f2 w0 = tw3[tw3_at(j0, t)], w1 = tw3[tw3_at(j1, t)];
            postpair2(pw0, P0, Q0, w0, pw1, P1, Q1, w1);
            }
            if constexpr (SPEC && SPL) {
                const int a = j0 < 8 ? spl_a_lo : spl_a_hi, m = j0 < 8 ? spl_m_lo : spl_m_hi;
                pw[a + 32 * j0] = pw0.x;
                pw[m + 32 * (15 - j0)] = pw0.y;
                pw[a + 32 * j1] = pw1.x;
                pw[m + 32 * (15 - j1)] = pw1.y;
            } else if constexpr (SPEC) {
                ps[16 * j0] = pw0;
                ps[16 * j1] = pw1;
            } else {
                pv[2 * j0] = pw0.x;
                pv[2 * j0 + 1] = pw0.y;
                pv[2 * j1] = pw1.x;
                pv[2 * j1 + 1] = pw1.y;
            }
        });
        // lane 0's X[0] = Re Z[0] + Im Z[0] and X[512] = Re Z[0] - Im Z[0]
        f2 px;
        asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(px) : "v"(b[0]));
        px = px * px;
        const bool live = w < p.n_windows;
        float pk = -1.f;  // lanes t < K: tone t's power
        int arg = t < p.k ? t : kMaxTones;  // kMaxTones: this lane holds no tone
        if constexpr (SPEC) {
            if (l0) {
                if constexpr (SPL) {
                    pw[rowb] = px.x;
                    pw[rowb + 512] = px.y;
                } else {
                    pq[512] = px.x;
                    pq[513] = px.y;
                }
            }
            wave_sync();
            // 5. tone pick from the slab
            if (t < p.k) pk = SPL ? pw[rowb + mybin] : pq[myslot];
            // SPL: the fenced lane id again, so the store address is formed
            // here rather than held across the loop
            if (live && t < p.k && p.mag) p.mag[w * p.k + (SPL ? tt : t)] = pk;
        } else {
            // 5. tone pick, gathered: tone i's power sits in lane
            //    (slot >> 1) & 15 of each window row at pv[slot >> 5 | half]
            //    (p.slot: a uniform index) and is read across the row with
            //    one ds_bpermute into lane t = i, so lanes t < K end holding
            //    tone t's power, as the slab pick of the spectrum path leaves
            //    them: one coalesced magnitude store and the same row argmax
            float mine = -1.f;
#pragma nounroll
            for (int i = 0; i < p.k; ++i) {
                const int f = p.slot[i];
                const float v = f >= 512 ? (f == 512 ? px.x : px.y) : pv[((f >> 5) << 1) | (f & 1)];
                const int src = f >= 512 ? 0 : ((f >> 1) & 15);
                const float got = __int_as_float(
                    __builtin_amdgcn_ds_bpermute(rowaddr + 4 * src, __float_as_int(v)));
                mine = t == i ? got : mine;
            }
            pk = mine;
            if (live && t < p.k && p.mag) p.mag[w * p.k + t] = pk;
        }
        // row argmax, ties to the lowest tone: the two DPP max passes of
        // window_sum.h (powers >= 0, so their bits order as unsigned)
        const bool owns = arg < kMaxTones;
        float mx;
        arg = (int)ws_argmax_m<false>(__float_as_uint(pk), owns, arg, 0u, false, 0, mx);
        // decision rescue, two stages: the int16 worst case,
        // then (only waves with a stage-1 flag) the window's energy by
        // Parseval, E = 2 x the sum of its 513 bin powers >= n sum x^2 (the
        // row's lanes hold every bin once, bin 256 twice in the register
        // tuple: an upper bound either way)
        auto efn = [&]() {
            float e = 0.f;
            if constexpr (SPEC && SPL) {
                // the fenced lane id again (as the stores below): the row
                // base is not kept live from the post-pass
                int tl2 = (int)(threadIdx.x & 63);
                asm volatile("" : "+v"(tl2));
                const float *row = pw + (tl2 >> 4) * 513;
                for (int i = tl2 & 15; i < 513; i += 16) e += row[i];
            } else if constexpr (SPEC) {
                for (int i = t; i < 513; i += 16) e += pq[quad_slot(i)];
            } else if constexpr (PICK == 2) {
                // not every bin's power exists here: n sum x^2 from the
                // window's samples, read again (L2; only waves stage 1
                // flagged), lane t's 64 (dwords t + 16 n1)
                if (live) {
                    const uint32_t *src = reinterpret_cast<const uint32_t *>(p.pcm + w * p.hop) + t;
#pragma unroll
                    for (int n1 = 0; n1 < 32; ++n1) {
                        const uint32_t d = src[16 * n1];
                        const float lo = (float)(int16_t)(d & 0xFFFFu), hi = (float)(int16_t)(d >> 16);
                        e = __builtin_fmaf(lo, lo, e);
                        e = __builtin_fmaf(hi, hi, e);
                    }
                }
                return 1024.f * row_sum16(e);
            } else {
                f2 a = {0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 32; i += 2) a = a + f2{pv[i], pv[i + 1]};
                e = (a.x + a.y) + (l0 ? px.x + px.y : 0.f);
            }
            return 2.f * row_sum16(e);
        };
        const bool amb = p.k >= 2 && ws_amb_two_stage(mx, pk, owns, 0.f, false, live, p.amb_tq,
                                                      p.amb_floor, p.amb_t2e, efn);
        if (live && t == 0) p.sym[w] = (uint8_t)(arg | (amb ? kSymAmbiguous : 0));
        if constexpr (SPEC && SPL) {
            if (p.spec) {
                // the group's live windows: floats [0, L) of the slab = the
                // output run from window 4 g (16-byte aligned: 4 g x 513 x 4 B)
                const long long wg = 4 * g;
                const int L = 513 * (int)(p.n_windows - wg < 4 ? p.n_windows - wg : 4);
                float *dst = p.spec + wg * 513;
                const f4 *src4 = reinterpret_cast<const f4 *>(pw);
#pragma unroll
                for (int i = 0; i < 9; ++i) {
                    const int f = 64 * i + lane;
                    if (4 * f + 4 <= L) {
                        __builtin_nontemporal_store(src4[f], reinterpret_cast<f4 *>(dst + 4 * f));
                    } else if (4 * f < L) {
                        for (int e = 4 * f; e < L; ++e) dst[e] = pw[e];
                    }
                }
            }
        } else if constexpr (SPEC) {
            if (p.spec && live) {
                float *so = p.spec + w * 513;
                for (int i = t; i < 513; i += 16) so[i] = pq[quad_slot(i)];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }

    // 6. decision rescue (rescue_fft.h), after the group loop
    //    (no code inside it, whose registers stay as they were): the symbol
    //    bytes of the groups are read back (one byte per window, plain loads:
    //    the bytes were written by this wave or its block) and every
    //    flagged window is decided again in double, one window per wave at a
    //    time through the wave's slab.
    //    Each wave takes its own groups' windows.
    auto rescue_one = [&](long long ww, lds_double *xs) {
        rescue_fft_window(p.pcm + ww * p.hop, xs, reinterpret_cast<const double2 *>(p.rtw), p.bins, p.k,
                          p.sym + ww, p.mag ? p.mag + ww * p.k : nullptr, p.spec ? p.spec + ww * 513 : nullptr);
    };
    auto flags4 = [&](long long gl) {  // bit q: window 4 gl + q is flagged
        unsigned f = 0;
        if (gl < n_groups) {
#pragma unroll
            for (int q0 = 0; q0 < 4; ++q0) {
                const long long ww = 4 * gl + q0;
                if (ww < p.n_windows && (p.sym[ww] & kSymAmbiguous)) f |= 1u << q0;
            }
        }
        return f;
    };
    if (p.rescue) {
        // this wave's symbol stores have landed (in this XCD's L2, where
        // the plain loads below find them) and are ordered before the loads
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        lds_double *xs = (lds_double *)(slab[wave]);
        bool rescan = true;  // the double FFTs' scan (below) has work
        if (p.t2e64 > 0.0 && !p.spec) {
            // first pass over each flagged group's windows, one per row
            // (rescue_fft_seg), where it is cheaper than their double
            // FFTs: it costs ~k x 200 double operations per lane for the
            // whole group, a double FFT ~800 per flagged window (at k = 8
            // and ~1.8 flagged windows per group both cost the same,
            // profiles/round4/r4l/). It clears the flag of every window
            // it decides; the loop below then finds only what it left.
            // (A separate loop: folded into the one below it made that
            // loop's double FFTs 30 % slower, profiles/round4/r4n/.)
            // (a wave that finds no flagged window here, nearly all of
            // them, skips the second scan of its symbol bytes)
            bool any = false;
            for (long long gb = g_first; gb < n_groups; gb += 64 * stride) {
                const unsigned f = flags4(gb + (long long)lane * stride);
                unsigned long long m = __ballot(f != 0);
                any = any || m != 0;
                while (m) {
                    const int src = __builtin_ctzll(m);
                    m &= m - 1;
                    const unsigned fs = (unsigned)__builtin_amdgcn_readlane((int)f, src);
                    if (p.k > 4 * __builtin_popcount(fs)) continue;
                    const long long gs = gb + (long long)src * stride;
                    const int row = lane >> 4;
                    const long long ww = 4 * gs + row;
                    const bool amb = (fs >> row) & 1u;
                    (void)rescue_fft_seg(p.pcm + (amb ? ww : 0) * p.hop, p.rot64, p.t2e64, p.k, lane & 15,
                                         amb, p.sym + ww, p.mag ? p.mag + ww * p.k : nullptr, p.fold64 != 0);
                }
            }
            __builtin_amdgcn_s_waitcnt(0);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            rescan = any;
        }
        for (long long gb = g_first; rescan && gb < n_groups; gb += 64 * stride) {
            const unsigned f = flags4(gb + (long long)lane * stride);
            unsigned long long m = __ballot(f != 0);
            while (m) {
                const int src = __builtin_ctzll(m);
                m &= m - 1;
                const unsigned fs = (unsigned)__builtin_amdgcn_readlane((int)f, src);
                const long long gs = gb + (long long)src * stride;
                for (int q0 = 0; q0 < 4; ++q0)
                    if ((fs >> q0) & 1u) rescue_one(4 * gs + q0, xs);
            }
        }
    }
}

// (The body stays a function of its own, taking the parameter block by
// reference: written straight into the kernel, the compiler orders its scalar
// loads differently.)
template <bool SPEC, int AUX, int SPL = 0, int OVL = 0, int PICK = 0>
__global__ __launch_bounds__(64 * 4) __attribute__((amdgpu_waves_per_eu(4)))
void fft1024_quad_kernel(FftParams p)
{
    fft1024_quad_body<SPEC, AUX, SPL, OVL, PICK>(p);
}

// Persistent grid: as many blocks as fit the chip, each wave strides over
// groups of 4 windows (the LDS twiddle tables are built once per block).
template <bool SPEC, int AUX, int SPL = 0, int OVL = 0, int PICK = 0>
hipError_t launch_fft_quad_t(const FftParams &p, hipStream_t s)
{
    constexpr int WPB = 4;
    void (*kern)(FftParams) = fft1024_quad_kernel<SPEC, AUX, SPL, OVL, PICK>;
    int dev = 0, cus = 256, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * WPB, 0) != hipSuccess || per_cu < 1)
        per_cu = 1;
    const long long groups = (p.n_windows + 3) / 4;
    long long blocks = (groups + WPB - 1) / WPB;
    blocks = std::min<long long>(blocks, (long long)cus * per_cu);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64 * WPB), 0, s, p);
    return hipGetLastError();
}

// What ships: 4-wave blocks, 4 waves/SIMD, loads at the top of each group
// (scripts/fft_probe.hip, profiles/round2/fft/). Load policy: windows that
// overlap (hop < n) are read by up to n / hop groups, so their loads keep the
// lines in L2 (plain cached loads, AUX 0: FETCH 1.06x the stream at hop 256,
// 3-6 % faster; sc0 measured the same or slower); disjoint windows stream
// through with nt (AUX 2; nt at hop 256 re-fetches 1.55x the stream).
// The DFT-4 stages (stage 2: two interleaved per block), the DFT-32's trivial
// pieces and the post-pass pairs are single asm blocks (probe FUSED 4:
// -3 to -4.5 % at hop 256, -2 to -4 % at hop 1024 against separate blocks;
// scripts/fft_probe.hip, profiles/round2/fft_fused/).
// The full-spectrum store (p.spec) goes through the linear slab with
// non-temporal 16-byte stores (SPL 2) when the output is 16-byte aligned,
// else through the quad_slot slab. Hop 256, 4.19 M windows, 8.6 GB of
// spectrum: quad_slot slab 4.00-4.12 ms, linear slab 2.85-2.89 ms, + nt
// 2.73 ms; a write-only fill of the same buffer 1.45 ms, the detector
// without the spectrum 1.71-1.80 ms (scripts/spectrum_probe.py,
// profiles/round2/spec_lin/).
// Tones only: the gathered tone pick (PICK 1), -1.8 % at hop 256 and -1.7 %
// at hop 1024 against the per-lane register pick, identical outputs
// (profiles/round3/r3s/); round 5: only the post-pass blocks holding a tone
// bin (PICK 2, -13 %), with round 1 of the transpose overlapping column 0's
// DFT-16 (OVL: within +-0.5 % on the full post-pass, -2.7 % once the VALU
// stream had shrunk; profiles/round5/r5zp/).
//                                          <SPEC, AUX, SPL, OVL, PICK>
hipError_t launch_fft_quad(const FftParams &p, hipStream_t s)
{
    const bool lin = p.spec && ((uintptr_t)p.spec & 15) == 0;
    if (p.hop < 1024) {
        if (lin) return launch_fft_quad_t<true, 0, 2>(p, s);
        if (p.spec) return launch_fft_quad_t<true, 0>(p, s);
        return p.pmask == 0xFFu ? launch_fft_quad_t<false, 0, 0, 0, 1>(p, s)
                                : launch_fft_quad_t<false, 0, 0, 1, 2>(p, s);
    }
    if (lin) return launch_fft_quad_t<true, 2, 2>(p, s);
    if (p.spec) return launch_fft_quad_t<true, 2>(p, s);
    return p.pmask == 0xFFu ? launch_fft_quad_t<false, 2, 0, 0, 1>(p, s)
                            : launch_fft_quad_t<false, 2, 0, 1, 2>(p, s);
}

int fft_quad_slot(int bin) { return quad_slot(bin); }

// The post-pass pair blocks (pairs 2 jb, 2 jb + 1) the tone bins sit in
// (quad_slot: pair j = slot >> 5; bins 0 and 512 come from Z[0] on the side)
unsigned fft_quad_pmask(const int *bins, int k)
{
    unsigned m = 0;
    for (int i = 0; i < k; ++i) {
        const int f = quad_slot(bins[i]);
        if (f < 512) m |= 1u << ((f >> 5) >> 1);
    }
    return m;
}

}  // namespace fskd
