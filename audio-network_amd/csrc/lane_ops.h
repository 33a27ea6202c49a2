// lane_ops.h — the small device pieces the kernel files share: vector
// typedefs, the DPP move and lane-group sum, the wave-level LDS sync, the
// tile's clamped buffer resource with its eight 16-byte loads, and (host side)
// the run-time tone count -> template instantiation switch.
// Every kernel file is its own translation unit; this is the one copy.
// What looks alike but stays in the kernels: each tile's chunk-offset table
// (and fft_quad.hip's group resource), because the shipped kernels' machine
// code changes when those go through a function (scripts/kernel_isa_diff.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace fskd {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}

// Sum over aligned groups of 2^log2g lanes; every lane of a group gets the
// bit-identical total (each step adds the same two operands in both lanes).
__device__ __forceinline__ float group_sum(float v, int log2g)
{
    if (log2g > 0) v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2]: lane ^ 1
    if (log2g > 1) v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1]: lane ^ 2
    if (log2g > 2) v += dpp_f<0x141>(v);  // row_half_mirror: other quad of the 8
    if (log2g > 3) v += dpp_f<0x140>(v);  // row_mirror: other half of the row
    if (log2g > 4) v += __shfl_xor(v, 16);
    if (log2g > 5) v += __shfl_xor(v, 32);
    return v;
}

// The wave's LDS writes before, its LDS reads after (a wave-private slice
// needs no block barrier).
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Buffer resource of the windows from `wbase` to the batch's end (windows of n
// samples every `hop`), clamped to the 2 GiB a record count holds: loads past
// the last window's last sample return zero instead of faulting. P: the
// kernel's parameter block (GoertzelParams, FftParams: pcm, n_windows, hop),
// read here in the order the kernels read it when this stood inline in each
// of them; the shipped kernels' instruction schedule depends on that order.
template <typename P>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const P &p, long long wbase, int n)
{
    long long bytes = ((p.n_windows - wbase - 1) * p.hop + n) * 2;
    if (bytes > 0x7FFFFFF0LL) bytes = 0x7FFFFFF0LL;
    return __builtin_amdgcn_make_buffer_rsrc((void *)(p.pcm + wbase * p.hop), (short)0, (int)bytes, 0x00020000);
}

// A tile's eight 16-byte loads at this lane's byte offsets; AUX: the
// cache-policy bits (2 = non-temporal, 0 = plain).
template <int AUX>
__device__ __forceinline__ void tile_load(__amdgpu_buffer_rsrc_t rs, const int (&goff)[8], u32x4 (&v)[8])
{
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, goff[i], 0, AUX);
}

// Host: f(std::integral_constant<int, K>{}) for the run-time tone count k in
// 1..kMaxTones (a kernel pointer), nullptr for any other k.
template <typename F>
const void *for_tone_count(int k, F &&f)
{
    switch (k) {
#define FSKD_CASE(K) case K: return f(std::integral_constant<int, K>{});
        FSKD_CASE(1) FSKD_CASE(2) FSKD_CASE(3) FSKD_CASE(4)
        FSKD_CASE(5) FSKD_CASE(6) FSKD_CASE(7) FSKD_CASE(8)
        FSKD_CASE(9) FSKD_CASE(10) FSKD_CASE(11) FSKD_CASE(12)
        FSKD_CASE(13) FSKD_CASE(14) FSKD_CASE(15) FSKD_CASE(16)
#undef FSKD_CASE
    default: return nullptr;
    }
}

}  // namespace fskd
