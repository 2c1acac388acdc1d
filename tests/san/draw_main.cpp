// TEST INFRASTRUCTURE ONLY — a stand-alone program for the AddressSanitizer / UBSan objects of the CPU logic build (make draw-san): the per-row
// draws of csrc/draw.hip through ssdr_draw_perm_dev, ssdr_draw_uniform_dev and ssdr_draw_normal_dev alone.
// In the CPU logic build device memory is host memory: every output is a std::vector of exactly the size the entry is promised, so an access one
// element off is a report.  Results are compared with a scalar restatement of the chain in include/ssdr_al.h: permutations and uniforms bit for
// bit, normals bit for bit as well (the same libm on both sides).  Run it as tests/test_sanitizers.py runs its programs, with
// ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0: the CPU build keeps its fibre stacks for the life of its worker threads.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/ssdr_al.h"

namespace {
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, ssdr_last_error()); return 1; } \
    } while (0)

uint32_t mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
struct Counter { uint64_t seed; uint32_t epoch, step, kind; };
uint32_t chain(const Counter& c, uint32_t lane, uint64_t e, uint32_t j) {
    uint32_t s = mix((uint32_t)c.seed ^ lane);
    s = mix(s ^ (uint32_t)(c.seed >> 32)); s = mix(s ^ c.epoch); s = mix(s ^ c.step); s = mix(s ^ c.kind);
    s = mix(s ^ (uint32_t)e); s = mix(s + (uint32_t)(e >> 32)); s = mix(s ^ j);
    return s;
}
uint32_t word(const Counter& c, uint64_t e, uint32_t j) { return mix(chain(c, 0x9e3779b9u, e, j) + chain(c, 0x85ebca6bu, e, j)); }
uint64_t bits53(const Counter& c, uint64_t e, uint32_t j) { return (uint64_t)(word(c, e, j) >> 5) * (1ull << 26) + (word(c, e, j + 1) >> 6); }

int perm_case(uint64_t seed, uint32_t epoch, uint32_t step, uint64_t first_tile, size_t B, size_t N, int key_bits) {
    const Counter c{seed, epoch, step, SSDR_DRAW_PERM};
    std::vector<int32_t> got(B * N, -1), want(B * N);
    for (size_t t = 0; t < B; ++t) {
        std::vector<uint32_t> key(N);
        for (size_t r = 0; r < N; ++r) key[r] = word(c, ((first_tile + t) << 32) | r, 0) >> (32 - key_bits);
        int32_t* row = want.data() + t * N;
        for (size_t r = 0; r < N; ++r) row[r] = (int32_t)r;
        std::stable_sort(row, row + N, [&](int32_t a, int32_t b) { return key[a] < key[b]; });
    }
    CHECK(ssdr_draw_perm_dev(seed, epoch, step, first_tile, B, N, key_bits, got.data(), nullptr) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    CHECK(std::memcmp(got.data(), want.data(), 4 * got.size()) == 0);
    std::printf("perm %zu x %zu, first tile %llu, %d key bits: ok\n", B, N, (unsigned long long)first_tile, key_bits);
    return 0;
}

int uniform_case(uint64_t seed, uint64_t first, size_t n) {
    const Counter c{seed, 2, 5, SSDR_DRAW_DUP};
    std::vector<float> got(n, -1.f), want(n);
    for (size_t i = 0; i < n; ++i) want[i] = (float)(word(c, first + i, 0) >> 8) * 0x1p-24f;
    CHECK(ssdr_draw_uniform_dev(seed, c.epoch, c.step, c.kind, first, n, got.data(), nullptr) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    CHECK(std::memcmp(got.data(), want.data(), 4 * n) == 0);
    for (float v : got) CHECK(v >= 0.f && v < 1.f);
    std::printf("uniform %zu from %llu: ok\n", n, (unsigned long long)first);
    return 0;
}

int normal_case(uint64_t seed, uint64_t first, size_t n, double scale) {
    const Counter c{seed, 7, 1, SSDR_DRAW_AUG_NOISE};
    std::vector<double> got(n, -1.0), want(n);
    for (size_t i = 0; i < n; ++i) {
        const double u1 = (double)(bits53(c, first + i, 0) + 1ull) * 0x1p-53, u2 = (double)bits53(c, first + i, 2) * 0x1p-53;
        const double rad = std::sqrt(-2.0 * std::log(u1));
        const double z = rad * std::cos(6.283185307179586 * u2);
        want[i] = scale * z;
    }
    CHECK(ssdr_draw_normal_dev(seed, c.epoch, c.step, c.kind, first, n, scale, got.data(), nullptr) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    CHECK(std::memcmp(got.data(), want.data(), 8 * n) == 0);
    std::printf("normal %zu from %llu, scale %g: ok\n", n, (unsigned long long)first, scale);
    return 0;
}
}  // namespace

int main() {
    CHECK(ssdr_init(0) == SSDR_OK);
    const uint64_t seed = 0xfedcba9876543210ull;
    if (perm_case(seed, 0, 0, 0, 1, 1, 32)) return 1;
    if (perm_case(seed, 1, 2, 0, 3, 2047, 32)) return 1;                // the sort tile's edges: a segment of one tile less one pair ...
    if (perm_case(seed, 1, 2, 0, 2, 2048, 32)) return 1;                // ... exactly one tile ...
    if (perm_case(seed, 1, 2, 0, 3, 2049, 32)) return 1;                // ... and one pair more: padded to two
    if (perm_case(seed, 3, 4, 2, 5, 4097, 32)) return 1;
    if (perm_case(seed, 3, 4, 0, 3, 5000, 4)) return 1;                 // ties everywhere
    if (perm_case(seed, 5, 6, 7, 70, 1100, 32)) return 1;               // more segments than one round of the sort takes (64)
    if (perm_case(seed, 5, 6, 0, 300, 7, 32)) return 1;                 // small tiles share a segment: 2100 pairs, two sort tiles
    if (perm_case(seed, 5, 6, 0, 2, 1024, 32)) return 1;                // the largest tiles that share, exactly one sort tile
    if (perm_case(seed, 8, 9, 0, 2, 40960, 32)) return 1;               // the workload's tile
    if (perm_case(seed, 8, 9, 0xffffffffull, 1, 33, 32)) return 1;      // the last tile id
    if (uniform_case(seed, 0, 1)) return 1;
    if (uniform_case(seed, 3, 255)) return 1;
    if (uniform_case(seed, 0xfffffff0ull, 600)) return 1;               // across the element's high word, more than two blocks
    if (uniform_case(seed, 0, 2048 * 256 + 1)) return 1;                // one element more than the capped grid covers in one stride
    if (normal_case(seed, 0, 1, 1.0)) return 1;
    if (normal_case(seed, 5, 3 * 1029, 0.001)) return 1;
    if (normal_case(seed, 0xffffffffull, 2048 * 256 + 1, 1.0)) return 1;
    {   // refused before anything is launched: the one-element arrays stay as they are
        std::vector<int32_t> p(1, -7); std::vector<float> u(1, -7.f); std::vector<double> z(1, -7.0);
        CHECK(ssdr_draw_perm_dev(1, 0, 0, 0, 1, 1, 32, nullptr, nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_draw_perm_dev(1, 0, 0, 0, 0, 8, 32, p.data(), nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_draw_perm_dev(1, 0, 0, 0, 8, 0, 32, p.data(), nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_draw_perm_dev(1, 0, 0, 0, 8, 8, 0, p.data(), nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_draw_perm_dev(1, 0, 0, 0, 8, 8, 33, p.data(), nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_draw_perm_dev(1, 0, 0, 0xffffffffull, 2, 8, 32, p.data(), nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_draw_perm_dev(1, 0, 0, 0, (size_t)1 << 19, 2049, 32, p.data(), nullptr) == SSDR_ERR_UNSUPPORTED);
        CHECK(ssdr_draw_uniform_dev(1, 0, 0, 1, 0, 0, u.data(), nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_draw_uniform_dev(1, 0, 0, 1, 0, 1, nullptr, nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_draw_normal_dev(1, 0, 0, 2, 0, 0, 1.0, z.data(), nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_draw_normal_dev(1, 0, 0, 2, 0, 1, 1.0, nullptr, nullptr) == SSDR_ERR_INVALID);
        CHECK(p[0] == -7 && u[0] == -7.f && z[0] == -7.0);
    }
    std::printf("draw ok\n");
    return 0;
}
