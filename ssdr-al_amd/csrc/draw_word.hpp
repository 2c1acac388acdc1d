// The counter-based chain behind every device-side draw (include/ssdr_al.h, "per-row draws"): draw_word is that statement in code, shared by the
// generators' per-row draws (draw.hip) and the region samplers (select_random.hip).
#pragma once
#include "mix32.hpp"

namespace ssdr {

constexpr uint32_t DRAW_LANE0 = 0x9e3779b9u, DRAW_LANE1 = 0x85ebca6bu;

// the part of the chain that is the same for every element of a call
struct DrawBase { uint32_t s0, s1; };
inline DrawBase draw_base(uint64_t seed, uint32_t epoch, uint32_t step, uint32_t kind) {
    DrawBase b;
    uint32_t* out[2] = {&b.s0, &b.s1};
    const uint32_t lane[2] = {DRAW_LANE0, DRAW_LANE1};
    for (int l = 0; l < 2; ++l) {
        uint32_t s = mix32((uint32_t)seed ^ lane[l]);
        s = mix32(s ^ (uint32_t)(seed >> 32)); s = mix32(s ^ epoch); s = mix32(s ^ step); s = mix32(s ^ kind);
        *out[l] = s;
    }
    return b;
}
// word j of element e: two chains that differ in their first constant, added and mixed once more (one chain alone is a bijection of the low
// word of e: the keys of a tile would be one fixed bijection of an aligned block of integers)
__device__ __forceinline__ uint32_t draw_word(DrawBase b, uint64_t e, uint32_t j) {
    const uint32_t lo = (uint32_t)e, hi = (uint32_t)(e >> 32);
    uint32_t a = mix32(b.s0 ^ lo); a = mix32(a + hi); a = mix32(a ^ j);
    uint32_t c = mix32(b.s1 ^ lo); c = mix32(c + hi); c = mix32(c ^ j);
    return mix32(a + c);
}

}  // namespace ssdr
