// TEST INFRASTRUCTURE ONLY — a stand-alone program for the AddressSanitizer / UBSan objects of the CPU logic build (make region-draw-sharded-san): the
// sharded draw of csrc/select_random.hip in its two halves, ssdr_region_draw_count_dev and ssdr_region_draw_sharded_dev, with two ranks emulated in one
// process (a copy of the ranks' count tables stands in for the all-gather).  In the CPU logic build device memory is host memory: every array is a
// std::vector of exactly the size the entry is promised — a rank's item list and position list hold exactly its share — so an access one element off is a
// report.  Merged by position, the ranks' items are compared with a scalar restatement of the rule in include/ssdr_al.h over the union.  Run it with
// ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0: the CPU build keeps its fibre stacks for the life of its threads.
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

struct Rank { std::vector<uint8_t> labeled; std::vector<int32_t> cloud; size_t B, first; };

// shares[r]: the region counts of rank r's clouds; every `step`-th region of the union is labelled
int sharded_case(const std::vector<std::vector<int>>& shares, int step, int64_t k, int key_bits) {
    const uint64_t seed = 0x0123456789abcdefull; const uint32_t rnd = 3, it = 1;
    const size_t W = shares.size();
    std::vector<Rank> ranks(W);
    std::vector<std::vector<int32_t>> unl;                     // per global cloud: its unlabelled regions as ids of the union
    std::vector<size_t> rank_of;                               // the rank of every global cloud
    size_t g = 0, CS = 0;
    for (size_t r = 0; r < W; ++r) {
        Rank& R = ranks[r]; R.B = shares[r].size(); R.first = g; CS = std::max(CS, R.B);
        for (size_t c = 0; c < R.B; ++c) {
            unl.emplace_back(); rank_of.push_back(r);
            for (int i = 0; i < shares[r][c]; ++i, ++g) {
                const bool lab = step && (g + 1) % (size_t)step == 0;
                R.cloud.push_back((int32_t)c); R.labeled.push_back(lab ? 1 : 0);
                if (!lab) unl.back().push_back((int32_t)g);
            }
        }
    }
    const size_t T = g;
    // the rule over the union, scalar
    std::vector<size_t> live;
    for (size_t c = 0; c < unl.size(); ++c) if (!unl[c].empty()) live.push_back(c);
    const size_t L = live.size();
    std::vector<int32_t> each(L, 0);
    std::vector<std::vector<int32_t>> want(W), want_pos(W);    // per rank: its items (ids of the union) and their positions in the union's list
    int64_t remain = 0, at = 0, left = 0;
    const Counter c3{seed, rnd, it, SSDR_DRAW_REGION_COUNT}, c4{seed, rnd, it, SSDR_DRAW_REGION_PICK};
    std::vector<uint32_t> key(T); std::vector<int64_t> e(T);
    for (size_t i = 0; i < T; ++i) { key[i] = word(c3, i, 0) >> (32 - key_bits); e[i] = (int64_t)i; }
    std::stable_sort(e.begin(), e.end(), [&](int64_t a, int64_t b) { return key[a] < key[b]; });
    for (int64_t i = 0; i < k; ++i) each[e[i] % (int64_t)L] += 1;
    for (size_t d = 0; d < L; ++d) {
        std::vector<int32_t> u = unl[live[d]];
        left += (int64_t)u.size();
        if (each[d] == 0) continue;
        size_t take = (size_t)each[d];
        if (take > u.size()) { remain += each[d] - (int64_t)u.size(); take = u.size(); }
        else std::stable_sort(u.begin(), u.end(), [&](int32_t a, int32_t b) { return (word(c4, (uint64_t)a, 0) >> (32 - key_bits)) < (word(c4, (uint64_t)b, 0) >> (32 - key_bits)); });
        for (size_t i = 0; i < take; ++i, ++at) { want[rank_of[live[d]]].push_back(u[i]); want_pos[rank_of[live[d]]].push_back((int32_t)at); }
    }
    left -= at;
    // the first half on every rank, the tables side by side as the all-gather leaves them
    std::vector<int32_t> u_all(W * (CS + 1), -1);
    for (size_t r = 0; r < W; ++r) {
        std::vector<int32_t> u(CS + 1, -1);
        CHECK(ssdr_region_draw_count_dev(ranks[r].labeled.data(), ranks[r].cloud.data(), ranks[r].cloud.size(), ranks[r].B, u.data(), CS, nullptr) == SSDR_OK);
        CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
        CHECK(u[CS] == 0);
        std::copy(u.begin(), u.end(), u_all.begin() + r * (CS + 1));
    }
    // the second half, over arrays of exactly the promised sizes
    for (size_t r = 0; r < W; ++r) {
        const Rank& R = ranks[r];
        std::vector<int32_t> items(want[r].size(), -1), pos(want[r].size(), -1), n_items(1, -1), shares_out(L, -1);
        std::vector<int64_t> count(1, k), info(8, -1);
        CHECK(ssdr_region_draw_sharded_dev(seed, rnd, it, SSDR_REGION_RANDOM, key_bits, R.first, (int)r, (int)W, u_all.data(), CS, R.labeled.data(), R.cloud.data(), R.cloud.size(),
                                           R.B, T, count.data(), items.data(), pos.data(), items.size(), n_items.data(), info.data(), nullptr) == SSDR_OK);
        CHECK(ssdr_region_draw_shares(nullptr, shares_out.data(), L) == SSDR_OK);
        CHECK(n_items[0] == (int32_t)want[r].size() && info[0] == (int64_t)L && info[1] == k && info[2] == at && info[3] == remain && info[4] == left && info[5] == 0 &&
              info[6] == (int64_t)want[r].size() && info[7] == 0);
        for (size_t i = 0; i < items.size(); ++i) CHECK(items[i] + (int32_t)R.first == want[r][i] && pos[i] == want_pos[r][i]);
        CHECK(std::memcmp(shares_out.data(), each.data(), 4 * L) == 0);
    }
    std::printf("sharded draw: %zu regions of %zu clouds (%zu live) on %zu ranks, %lld clicks, %d key bits -> %lld items (%zu + %zu), remainder %lld: ok\n", T, unl.size(), L, W,
                (long long)k, key_bits, (long long)at, want[0].size(), want[1].size(), (long long)remain);
    return 0;
}
}  // namespace

int main() {
    CHECK(ssdr_init(0) == SSDR_OK);
    if (sharded_case({{30, 25, 15}, {40, 21}}, 4, 50, 32)) return 1;      // 70 + 61 regions: rank 1's ids start at 70, no multiple of the wave
    if (sharded_case({{3, 2}, {1, 2, 3}}, 0, 11, 32)) return 1;           // click == total_num: a cloud is taken whole, the remainder is global
    {   // refused before anything is launched
        std::vector<uint8_t> lab(1, 0); std::vector<int32_t> cl(1, 0), u(2, -7), it(1, -7), ps(1, -7), n(1, -7); std::vector<int64_t> cnt(1, 1), info(8, -7);
        CHECK(ssdr_region_draw_count_dev(lab.data(), cl.data(), 1, 2, u.data(), 1, nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_region_draw_sharded_dev(1, 0, 0, 0, 32, 0, 0, 0, u.data(), 1, lab.data(), cl.data(), 1, 1, 1, cnt.data(), it.data(), ps.data(), 1, n.data(), info.data(),
                                           nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_region_draw_sharded_dev(1, 0, 0, 0, 32, 0, 1, 1, u.data(), 1, lab.data(), cl.data(), 1, 1, 1, cnt.data(), it.data(), ps.data(), 1, n.data(), info.data(),
                                           nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_region_draw_sharded_dev(1, 0, 0, 0, 32, 0x3fffffffull, 0, 1, u.data(), 1, lab.data(), cl.data(), 1, 1, 1, cnt.data(), it.data(), ps.data(), 1, n.data(),
                                           info.data(), nullptr) == SSDR_ERR_UNSUPPORTED);
        CHECK(u[0] == -7 && it[0] == -7 && ps[0] == -7 && n[0] == -7 && info[0] == -7);
    }
    std::printf("region draw sharded ok\n");
    return 0;
}
