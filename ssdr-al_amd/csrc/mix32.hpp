// The 32-bit mixer behind every counter-based draw of the library: the dropout mask (randla_train.hip) and the generators' per-row draws (draw.hip).
// A bijection of uint32, all arithmetic modulo 2^32.
#pragma once
#include <cstdint>

namespace ssdr {

__host__ __device__ inline uint32_t mix32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }

}  // namespace ssdr
