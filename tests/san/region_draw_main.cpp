// TEST INFRASTRUCTURE ONLY — a stand-alone program for the AddressSanitizer / UBSan objects of the CPU logic build (make region-draw-san): one case of
// each entry of csrc/select_random.hip — ssdr_region_draw_dev (random and label-all), ssdr_region_draw_shares and ssdr_seed_label_dev.
// In the CPU logic build device memory is host memory: every array is a std::vector of exactly the size the entry is promised, so an access one
// element off is a report.  The item lists are compared with a scalar restatement of the rule in include/ssdr_al.h.  Run it as tests/test_sanitizers.py
// runs its programs, with ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0: the CPU build keeps its fibre stacks for the life of its threads.
#include <algorithm>
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

// the regions of `sizes[c]` per cloud, every `step`-th labelled; -> the item list and each_file_number of one iteration
struct Pool { std::vector<uint8_t> labeled; std::vector<int32_t> cloud; size_t B; };
Pool make_pool(const std::vector<int>& sizes, int step) {
    Pool p; p.B = sizes.size();
    for (size_t c = 0; c < sizes.size(); ++c)
        for (int i = 0; i < sizes[c]; ++i) { p.cloud.push_back((int32_t)c); p.labeled.push_back(step && (int)p.cloud.size() % step == 0 ? 1 : 0); }
    return p;
}

int draw_case(const std::vector<int>& sizes, int step, int64_t k, size_t T, int key_bits, int mode) {
    const uint64_t seed = 0x0123456789abcdefull; const uint32_t rnd = 3, it = 1;
    Pool p = make_pool(sizes, step);
    const size_t S = p.cloud.size();
    // the rule, scalar
    std::vector<std::vector<int32_t>> unl(p.B);
    for (size_t s = 0; s < S; ++s) if (!p.labeled[s]) unl[p.cloud[s]].push_back((int32_t)s);
    std::vector<size_t> live;
    for (size_t c = 0; c < p.B; ++c) if (!unl[c].empty()) live.push_back(c);
    const size_t L = live.size();
    std::vector<int32_t> each(L, 0), want;
    int64_t remain = 0;
    if (mode == SSDR_REGION_ALL) {
        for (size_t d = 0; d < L; ++d) { each[d] = (int32_t)unl[live[d]].size(); want.insert(want.end(), unl[live[d]].begin(), unl[live[d]].end()); }
    } else {
        const Counter c3{seed, rnd, it, SSDR_DRAW_REGION_COUNT}, c4{seed, rnd, it, SSDR_DRAW_REGION_PICK};
        std::vector<uint32_t> key(T); std::vector<int64_t> e(T);
        for (size_t i = 0; i < T; ++i) { key[i] = word(c3, i, 0) >> (32 - key_bits); e[i] = (int64_t)i; }
        std::stable_sort(e.begin(), e.end(), [&](int64_t a, int64_t b) { return key[a] < key[b]; });
        for (int64_t i = 0; i < k; ++i) each[e[i] % (int64_t)L] += 1;
        for (size_t d = 0; d < L; ++d) {
            std::vector<int32_t> u = unl[live[d]];
            if (each[d] == 0) continue;
            if ((size_t)each[d] > u.size()) { remain += each[d] - (int64_t)u.size(); want.insert(want.end(), u.begin(), u.end()); continue; }
            std::stable_sort(u.begin(), u.end(), [&](int32_t a, int32_t b) { return (word(c4, (uint64_t)a, 0) >> (32 - key_bits)) < (word(c4, (uint64_t)b, 0) >> (32 - key_bits)); });
            want.insert(want.end(), u.begin(), u.begin() + each[d]);
        }
    }
    // the entry, over arrays of exactly the promised sizes
    std::vector<int32_t> items(want.size(), -1), n_items(1, -1), shares(L, -1);
    std::vector<int64_t> count(1, k), info(8, -1);
    CHECK(ssdr_region_draw_dev(seed, rnd, it, mode, key_bits, 0, p.labeled.data(), p.cloud.data(), S, p.B, T, count.data(), items.data(), items.size(), n_items.data(),
                               info.data(), nullptr) == SSDR_OK);
    CHECK(ssdr_region_draw_shares(nullptr, shares.data(), L) == SSDR_OK);
    CHECK(n_items[0] == (int32_t)want.size() && info[0] == (int64_t)L && info[2] == (int64_t)want.size() && info[3] == remain && info[5] == 0);
    CHECK(std::memcmp(items.data(), want.data(), 4 * want.size()) == 0);
    CHECK(std::memcmp(shares.data(), each.data(), 4 * L) == 0);
    std::printf("draw mode %d: %zu regions of %zu clouds (%zu live), %lld of %zu, %d key bits -> %zu items, remainder %lld: ok\n", mode, S, p.B, L, (long long)k, T, key_bits,
                want.size(), (long long)remain);
    return 0;
}

int seed_case() {
    // three regions: 3 points (the wave form), 300 points (the workgroup form), 0 points; the points are scattered over the cloud
    const size_t n = 310;
    std::vector<int32_t> gt(n), off = {0, 3, 303, 303}, pts(303), items = {1, 0, 2}, n_items = {3};
    for (size_t i = 0; i < n; ++i) gt[i] = (int32_t)(i * 7 % 13);
    for (size_t i = 0; i < 303; ++i) pts[i] = (int32_t)((i * 101) % n);
    std::vector<float> mask(n, 0.f), label(n, -1.f);
    std::vector<uint8_t> labeled(3, 0);
    std::vector<int64_t> out(3, -1);
    CHECK(ssdr_seed_label_dev(gt.data(), n, off.data(), pts.data(), 3, items.data(), n_items.data(), items.size(), 0, mask.data(), label.data(), labeled.data(), out.data(),
                              nullptr) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    CHECK(out[0] == 3 && out[1] == 303 && out[2] == 0 && labeled[0] && labeled[1] && labeled[2]);
    std::vector<char> hit(n, 0);
    for (int32_t q : pts) hit[q] = 1;
    for (size_t i = 0; i < n; ++i) CHECK(hit[i] ? (mask[i] == 1.f && label[i] == (float)gt[i]) : (mask[i] == 0.f && label[i] == -1.f));
    std::printf("seed label, both forms: ok\n");
    return 0;
}
}  // namespace

int main() {
    CHECK(ssdr_init(0) == SSDR_OK);
    if (draw_case({40, 1, 300, 7, 2500}, 5, 600, 2848, 32, SSDR_REGION_RANDOM)) return 1;      // more than one sort tile, two clouds taken whole
    if (draw_case({3, 2, 1, 2, 3}, 0, 11, 11, 4, SSDR_REGION_RANDOM)) return 1;                // click == total_num, ties everywhere
    if (draw_case({40, 1, 300, 7, 2500}, 3, 0, 1, 32, SSDR_REGION_ALL)) return 1;
    if (seed_case()) return 1;
    {   // refused before anything is launched
        std::vector<uint8_t> lab(1, 0); std::vector<int32_t> cl(1, 0), it(1, -7), n(1, -7); std::vector<int64_t> cnt(1, 1), info(8, -7);
        CHECK(ssdr_region_draw_dev(1, 0, 0, 0, 32, 0, nullptr, cl.data(), 1, 1, 1, cnt.data(), it.data(), 1, n.data(), info.data(), nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_region_draw_dev(1, 0, 0, 0, 32, 0, lab.data(), cl.data(), 0, 1, 1, cnt.data(), it.data(), 1, n.data(), info.data(), nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_region_draw_dev(1, 0, 0, 0, 32, 0, lab.data(), cl.data(), 1, 1, 0, cnt.data(), it.data(), 1, n.data(), info.data(), nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_region_draw_dev(1, 0, 0, 0, 33, 0, lab.data(), cl.data(), 1, 1, 1, cnt.data(), it.data(), 1, n.data(), info.data(), nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_seed_label_dev(nullptr, 1, cl.data(), cl.data(), 1, it.data(), n.data(), 1, 0, nullptr, nullptr, lab.data(), cnt.data(), nullptr) == SSDR_ERR_INVALID);
        CHECK(it[0] == -7 && n[0] == -7 && info[0] == -7);
    }
    std::printf("region draw ok\n");
    return 0;
}
