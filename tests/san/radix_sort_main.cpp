// TEST INFRASTRUCTURE ONLY — a stand-alone program for the AddressSanitizer / UBSan objects of the CPU logic build (make radix-sort-san): the radix sort of
// csrc/radix_sort.hip through ssdr_radix_sort_dev, one case of every group of tests/test_sort_paths.py.
// In the CPU logic build device memory is host memory: keys, values, counts and AND / OR words are std::vectors of exactly off[nseg], nseg and 2 * nseg
// elements, so an access one element off is a report.  Results are compared with std::stable_sort per segment, every slot: the dead slots behind a
// segment's live pairs keep what they held (the 0xA5 fill under SSDR_SORT_INPUT_IN_ALT).  Run it as tests/test_sanitizers.py runs its programs, with
// ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0: the CPU build keeps its fibre stacks for the life of its worker threads.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>
#include "../../include/ssdr_al.h"

namespace {
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, ssdr_last_error()); return 1; } \
    } while (0)

constexpr int TILE = 2048;
constexpr uint64_t DEAD_K = 0xdeadbeefcafef00dull, FILL_K = 0xa5a5a5a5a5a5a5a5ull;
constexpr uint32_t DEAD_V = 0xc0ffee11u, FILL_V = 0xa5a5a5a5u;

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }

struct Seg { int n; unsigned varying; int slack; };      // varying: bit p set = digit p of the key field varies
struct Case {
    const char* name;
    std::vector<Seg> segs;
    int key_bits = 64, shift = 0, flags = 0;
    bool kv = true, loose_words = false;
    std::vector<int> d_cnt;                                // empty: no device counts
    int distinct = 0;                                      // > 0: keys drawn from this many values (ties)
    int expect_npass = -1, expect_high = -1;
};

int run(const Case& c) {
    const int nseg = (int)c.segs.size();
    std::vector<int> off(nseg + 1, 0), n_host(nseg);
    for (int s = 0; s < nseg; ++s) { n_host[s] = c.segs[s].n; off[s + 1] = off[s] + ((c.segs[s].n + TILE - 1) / TILE + c.segs[s].slack) * TILE; }
    const uint64_t fmask = c.key_bits >= 64 ? ~0ull : (1ull << c.key_bits) - 1ull;
    std::vector<uint64_t> keys(off[nseg], DEAD_K), andor(2 * nseg);
    std::vector<uint32_t> vals(c.kv ? off[nseg] : 0, DEAD_V);
    std::vector<uint64_t> pool(std::max(c.distinct, 1));
    for (auto& p : pool) p = rnd();
    for (int s = 0; s < nseg; ++s) {
        uint64_t vmask = 0;
        for (int p = 0; p < 8; ++p) if (c.segs[s].varying >> p & 1) vmask |= 0xffull << (8 * p);
        vmask &= fmask;
        const uint64_t cst = rnd() & fmask & ~vmask;
        for (int i = 0; i < n_host[s]; ++i) {
            const uint64_t r = c.distinct > 0 ? pool[rnd() % c.distinct] : rnd();
            const uint64_t f = (r & vmask) | cst;
            keys[off[s] + i] = c.shift ? (f << c.shift) | ((uint64_t)i & ((1ull << c.shift) - 1ull)) : f;
            if (c.kv) vals[off[s] + i] = (uint32_t)(off[s] + i);
        }
    }
    const bool in_alt = (c.flags & SSDR_SORT_INPUT_IN_ALT) != 0;
    std::vector<uint64_t> want_k = in_alt ? std::vector<uint64_t>(keys.size(), FILL_K) : keys;
    std::vector<uint32_t> want_v = in_alt ? std::vector<uint32_t>(vals.size(), FILL_V) : vals;
    for (int s = 0; s < nseg; ++s) {
        const int cnt = std::max(0, c.d_cnt.empty() ? n_host[s] : std::min(c.d_cnt[s], n_host[s]));
        std::vector<int> order(cnt);
        std::iota(order.begin(), order.end(), 0);
        const uint64_t* k = keys.data() + off[s];
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return (k[a] >> c.shift) < (k[b] >> c.shift); });
        uint64_t a = ~0ull, o = 0ull;
        for (int i = 0; i < cnt; ++i) {
            want_k[off[s] + i] = k[order[i]];
            if (c.kv) want_v[off[s] + i] = vals[off[s] + order[i]];
            a &= k[i]; o |= k[i];
        }
        andor[2 * s] = a; andor[2 * s + 1] = o;
        if (c.loose_words && cnt > 0) { andor[2 * s] = 0; andor[2 * s + 1] = fmask << c.shift; }
    }
    std::vector<int> d_cnt = c.d_cnt;
    const bool words = c.loose_words;
    CHECK(ssdr_radix_sort_dev(keys.data(), c.kv ? vals.data() : nullptr, nseg, off.data(), n_host.data(), d_cnt.empty() ? nullptr : d_cnt.data(), c.key_bits,
                              c.shift, words ? andor.data() : nullptr, c.flags, nullptr) == SSDR_OK);
    int32_t rec[8];
    std::vector<uint64_t> used(2 * nseg, 7);
    CHECK(ssdr_radix_sort_info(nullptr, rec, used.data()) == SSDR_OK);
    CHECK(keys == want_k);
    CHECK(vals == want_v);
    CHECK(used == andor);                                  // the pre-pass found the words of the stable_sort side, or the given ones came through
    CHECK(rec[6] == off[nseg] / TILE && rec[7] == rec[6] + 1);
    if (c.expect_npass >= 0) CHECK(rec[0] == c.expect_npass);
    if (c.expect_high >= 0) CHECK(rec[2] == c.expect_high);
    std::printf("%s: ok (%d segments, %d slots, %d wide passes%s)\n", c.name, nseg, off[nseg], rec[0], rec[2] ? " + the one-workgroup kernel" : "");
    return 0;
}
}  // namespace

int main() {
    CHECK(ssdr_init(0) == SSDR_OK);
    const int ALT = SSDR_SORT_INPUT_IN_ALT, WIDE = SSDR_SORT_WIDE_HIGH;
    std::vector<Case> cases;
    auto add = [&](Case c) { cases.push_back(std::move(c)); return &cases.back(); };
    { Case c; c.name = "parity: two passes, home 0"; c.segs = {{3000, 0x21, 0}}; add(c); }
    { Case c; c.name = "parity: byte 7 alone, home 1"; c.segs = {{3000, 0x80, 0}}; c.flags = ALT; add(c); }
    { Case c; c.name = "parity: all keys equal, home 1, keys only"; c.segs = {{3000, 0, 0}}; c.flags = ALT; c.kv = false; add(c); }
    { Case c; c.name = "high passes in one workgroup"; c.segs = {{20000, 0x12, 0}}; c.key_bits = 40; c.expect_npass = 4; c.expect_high = 1; add(c); }
    { Case c; c.name = "high passes wide"; c.segs = {{16384, 0x30, 0}}; c.flags = WIDE; c.expect_npass = 8; c.expect_high = 0; add(c); }
    // rs_high_passes offsets its value pointer per segment: keys only there is no value array, and a null pointer takes no offset
    { Case c; c.name = "high passes, three segments, keys only"; c.segs = {{1025, 0x30, 1}, {2049, 0x20, 0}, {700, 0x82, 2}}; c.kv = false; add(c); }
    { Case c; c.name = "high passes, three segments, keys only, home 1"; c.segs = {{1025, 0x30, 1}, {2049, 0x20, 0}, {700, 0x82, 2}}; c.kv = false; c.flags = ALT; add(c); }
    { Case c; c.name = "high passes, three segments, values"; c.segs = {{1025, 0x30, 1}, {2049, 0x20, 0}, {700, 0x82, 2}}; add(c); }
    { Case c; c.name = "pre-pass: unrolled trip and tail"; c.segs = {{1025, 0x02, 0}}; c.key_bits = 32; add(c); }
    { Case c; c.name = "pre-pass: several blocks"; c.segs = {{5 * TILE + 77, 0x04, 0}}; c.key_bits = 32; add(c); }
    { Case c; c.name = "given words, the loosest, an empty segment"; c.segs = {{2500, 0x12, 0}, {0, 0, 1}, {5000, 0x12, 0}}; c.key_bits = 40; c.shift = 17; c.loose_words = true; add(c); }
    { Case c; c.name = "shift 32, keys only"; c.segs = {{5000, 0x0f, 0}}; c.key_bits = 32; c.shift = 32; c.kv = false; add(c); }
    { Case c; c.name = "shift 1, values"; c.segs = {{5000, 0xff, 0}}; c.key_bits = 63; c.shift = 1; c.flags = ALT; add(c); }
    {
        Case c; c.name = "64 segments of mixed counts"; c.key_bits = 32;
        const int mix[6] = {2049, 5000, 0, 1, 2047, 2048};
        for (int i = 0; i < 64; ++i) c.segs.push_back({mix[i % 6], i == 0 ? 0x05u : 0x01u, i % 3});
        add(c);
    }
    { Case c; c.name = "device counts"; c.segs = {{5000, 0x19, 0}, {2049, 0x19, 1}, {4101, 0x19, 0}, {3000, 0x19, 0}}; c.d_cnt = {100, 0, 1 << 30, 2999}; c.flags = ALT; add(c); }
    { Case c; c.name = "ties"; c.segs = {{10000, 0x0f, 0}}; c.key_bits = 32; c.distinct = 3; add(c); }
    { Case c; c.name = "scan carry: 257 tiles behind a small segment"; c.segs = {{3000, 0x02, 1}, {256 * TILE + 1, 0x02, 0}, {2500, 0x02, 0}}; c.key_bits = 32; add(c); }
    { Case c; c.name = "grid stride: 65 tiles, the last partial"; c.segs = {{64 * TILE + 777, 0x0a, 0}}; c.key_bits = 32; add(c); }
    { Case c; c.name = "small again"; c.segs = {{3000, 0x03, 0}}; c.key_bits = 32; add(c); }
    for (const Case& c : cases) if (run(c)) return 1;
    {   // refused before anything is touched
        std::vector<uint64_t> k(2 * TILE, 5); std::vector<uint32_t> v(2 * TILE, 6);
        std::vector<int> off66(66), n65(65, 1);
        for (int i = 0; i < 66; ++i) off66[i] = i * TILE;
        const int off[3] = {0, TILE, 2 * TILE}, odd[3] = {0, TILE - 1, 2 * TILE}, end[3] = {0, TILE, 2 * TILE - 1}, nh[2] = {100, 100}, big[2] = {100, TILE + 1}, zero[3] = {0, 0, 0};
        for (int flags : {0, ALT}) {
            CHECK(ssdr_radix_sort_dev(k.data(), v.data(), 65, off66.data(), n65.data(), nullptr, 64, 0, nullptr, flags, nullptr) == SSDR_ERR_INVALID);
            CHECK(ssdr_radix_sort_dev(k.data(), v.data(), 2, odd, nh, nullptr, 64, 0, nullptr, flags, nullptr) == SSDR_ERR_INVALID);
            CHECK(ssdr_radix_sort_dev(k.data(), v.data(), 2, end, nh, nullptr, 64, 0, nullptr, flags, nullptr) == SSDR_ERR_INVALID);
            CHECK(ssdr_radix_sort_dev(k.data(), v.data(), 2, off, big, nullptr, 64, 0, nullptr, flags, nullptr) == SSDR_ERR_INVALID);
            CHECK(ssdr_radix_sort_dev(k.data(), v.data(), 2, off, nh, nullptr, 64, -1, nullptr, flags, nullptr) == SSDR_ERR_INVALID);
            CHECK(ssdr_radix_sort_dev(k.data(), v.data(), 2, off, nh, nullptr, 64, 1, nullptr, flags, nullptr) == SSDR_ERR_INVALID);
            CHECK(ssdr_radix_sort_dev(k.data(), v.data(), 0, off, nh, nullptr, 64, 0, nullptr, flags, nullptr) == SSDR_OK);
            CHECK(ssdr_radix_sort_dev(k.data(), v.data(), 2, zero, zero, nullptr, 64, 0, nullptr, flags, nullptr) == SSDR_OK);
        }
        CHECK(ssdr_radix_sort_dev(k.data(), v.data(), 2, off, nh, nullptr, 64, 0, nullptr, 4, nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
        for (uint64_t x : k) CHECK(x == 5);
        for (uint32_t x : v) CHECK(x == 6);
    }
    std::printf("radix sort ok\n");
    return 0;
}
