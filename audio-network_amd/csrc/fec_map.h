/*
 * fec_map.h — the one copy of the map between the trellis's coded-bit index
 * and the position on the air (include/demod.h "coded frames": punctured and
 * interleaved), shared by frames_fec.hip, frames_tx.hip, frame_shape.h and
 * the host C (demod_fec.c). Plain integer code that compiles for both; only
 * constants are divided (the periods 2 and 3, the block of 256).
 *
 *  mother bit  m = 2 t + v, v = 0 generator 0171, v = 1 generator 0133
 *  puncturing  by step phase. Rate 2/3, period 2: phase 0 keeps v0 v1, phase 1
 *              v1. Rate 3/4, period 3: phase 0 keeps v0 v1, phase 1 v0, phase
 *              2 v1.
 *  code index  i = Nt(t) + the bit's rank among step t's kept bits
 *  air         a = i, or with DEMOD_FEC_INTERLEAVE i with the two nibbles of
 *              its low byte swapped (a 16 x 16 block, an involution)
 */
#ifndef FSKD_FEC_MAP_H
#define FSKD_FEC_MAP_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FEC_MAP_FN static __host__ __device__ __forceinline__
#else
#define FEC_MAP_FN static inline
#endif

#define FEC_MAP_NONE 0xFFFFFFFFu /* no such bit: punctured, or a pad position */

/* the six valid modes: 1 | {0, 0x10, 0x20} | {0, 0x40} */
FEC_MAP_FN int fec_mode_valid(unsigned fec)
{
    return (fec & 0xFu) == 1u && (fec & ~0x7Fu) == 0u && (fec & 0x30u) != 0x30u;
}

/* a mode whose map is not the identity */
FEC_MAP_FN int fec_mode_mapped(unsigned fec) { return (fec & 0x70u) != 0u; }

/* Nt(T): the kept bits of T steps */
FEC_MAP_FN unsigned fec_kept_bits(unsigned fec, unsigned T)
{
    if (fec & 0x10u) return 3u * (T / 2u) + 2u * (T % 2u);
    if (fec & 0x20u) {
        const unsigned r = T % 3u;
        return 4u * (T / 3u) + (r ? r + 1u : 0u);
    }
    return 2u * T;
}

/* St: the greatest T with Nt(T) <= Cu */
FEC_MAP_FN unsigned fec_steps_within(unsigned fec, unsigned Cu)
{
    if (fec & 0x10u) return 2u * (Cu / 3u) + (Cu % 3u == 2u ? 1u : 0u);
    if (fec & 0x20u) {
        const unsigned r = Cu % 4u;
        return 3u * (Cu / 4u) + (r ? r - 1u : 0u);
    }
    return Cu / 2u;
}

/* the air bits a row or frame of C bits uses: whole blocks with the flag */
FEC_MAP_FN unsigned fec_usable_bits(unsigned fec, unsigned C) { return (fec & 0x40u) ? C & ~255u : C; }

/* Na: Nt rounded up to whole blocks with the flag (Nt < 2^31) */
FEC_MAP_FN unsigned fec_air_bits(unsigned fec, unsigned Nt) { return (fec & 0x40u) ? (Nt + 255u) & ~255u : Nt; }

/* code index <-> air position: one function for both directions */
FEC_MAP_FN unsigned fec_interleave(unsigned fec, unsigned i)
{
    return (fec & 0x40u) ? (i & ~255u) | ((i & 15u) << 4) | ((i >> 4) & 15u) : i;
}

/* the code index of mother bit m, or FEC_MAP_NONE where it is punctured */
FEC_MAP_FN unsigned fec_code_index(unsigned fec, unsigned m)
{
    const unsigned t = m >> 1, v = m & 1u;
    if (fec & 0x10u) {
        const unsigned q = t / 2u;
        if (t - 2u * q) return v ? 3u * q + 2u : FEC_MAP_NONE;
        return 3u * q + v;
    }
    if (fec & 0x20u) {
        const unsigned q = t / 3u, ph = t - 3u * q;
        if (ph == 0u) return 4u * q + v;
        if (ph == 1u) return v ? FEC_MAP_NONE : 4u * q + 2u;
        return v ? 4u * q + 3u : FEC_MAP_NONE;
    }
    return m;
}

/* the mother bit of code index i */
FEC_MAP_FN unsigned fec_mother_bit(unsigned fec, unsigned i)
{
    if (fec & 0x10u) {
        const unsigned q = i / 3u, r = i - 3u * q;
        return 4u * q + (r == 2u ? 3u : r);
    }
    if (fec & 0x20u) {
        const unsigned q = i / 4u, r = i - 4u * q;
        return 6u * q + (r == 3u ? 5u : r);
    }
    return i;
}

/* the air position of mother bit m, or FEC_MAP_NONE */
FEC_MAP_FN unsigned fec_air_of_mother(unsigned fec, unsigned m)
{
    const unsigned i = fec_code_index(fec, m);
    return i == FEC_MAP_NONE ? i : fec_interleave(fec, i);
}

#endif
