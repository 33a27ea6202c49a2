// synth_ops.h — what the generator (synth.hip) and the transmitter's modulator
// (frames_tx.hip) share on the device: the splitmix64 finaliser behind every
// seeded value (DESIGN.md "Synthetic input").
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace fskd {

constexpr uint64_t kSynthGamma = 0x9E3779B97F4A7C15ULL;

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

}  // namespace fskd
