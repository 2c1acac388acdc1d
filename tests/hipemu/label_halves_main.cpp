// TEST INFRASTRUCTURE ONLY — a stand-alone program for the AddressSanitizer / UBSan objects of the CPU logic build (make label-halves-san): the
// labelling chain in two halves (ssdr_oracle_label_verdict_dev, ssdr_oracle_label_walk_dev) with three ranks emulated in one process against the
// one-call chain ssdr_oracle_label_dev over the union of the clouds, through the C ABI alone.  In the CPU logic build device memory is host memory:
// every array is a std::vector of exactly the size the entry is promised, so an access one element off is a report.
// Shapes as tests/test_sharded_labeling.py: ~2 200 picks, 1 000 record slots per rank (the scan crosses two 1 024-record chunks, dead slots lie
// between the ranks' live records), regions of 1, 255, 256, 257 and 5 000 points, a region picked twice, clouds of all ranks interleaved in the walk.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/ssdr_al.h"

namespace {
uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }
int rnd_below(int n) { return (int)(rnd() % (uint32_t)n); }

struct Clouds {
    std::vector<int32_t> gt, pred, sp_off{0}, sp_pts, sp_cloud;
    std::vector<int> first_region, first_point;      // per cloud (+ the end)
};

void add_region(Clouds& c, int cloud, int n) {
    const int p0 = (int)c.gt.size();
    const int base = rnd_below(13), cls = rnd_below(13), cut = n >= 8 && rnd_below(3) == 0 ? n / 2 : n;
    const int base2 = (base + 1 + rnd_below(12)) % 13, cls2 = (cls + 1 + rnd_below(12)) % 13;
    for (int i = 0; i < n; ++i) {
        const bool a = i < cut;
        c.gt.push_back(rnd_below(25) == 0 ? rnd_below(13) : (a ? base : base2));
        c.pred.push_back(rnd_below(20) == 0 ? rnd_below(13) : (a ? cls : cls2));
    }
    for (int i = 0; i < n; ++i) c.sp_pts.push_back(p0 + (n - 1 - i));      // (a region's points in descending order: not the identity)
    c.sp_off.push_back((int32_t)c.sp_pts.size());
    c.sp_cloud.push_back(cloud);
}

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, ssdr_last_error()); return 1; } \
    } while (0)
}  // namespace

int main() {
    const int B = 12, W = 3, PER = 190, MAXI = 1000, NL = 13, NC = 13;
    const int special[5] = {1, 255, 256, 257, 5000};
    Clouds u;
    for (int c = 0; c < B; ++c) {
        u.first_region.push_back((int)u.sp_cloud.size()); u.first_point.push_back((int)u.gt.size());
        for (int s = 0; s < PER; ++s) add_region(u, c, 3 + rnd_below(37));
        if (c == 1 || c == 6 || c == 10) for (int k = 0; k < 5; ++k) add_region(u, c, special[k]);
    }
    u.first_region.push_back((int)u.sp_cloud.size()); u.first_point.push_back((int)u.gt.size());
    const size_t n = u.gt.size(), S = u.sp_cloud.size();
    // picks: every special region, the 5 000-point one of cloud 6 twice, ~2 170 at random (repeats included), shuffled
    std::vector<int32_t> picks;
    for (int c : {1, 6, 10}) for (int k = 0; k < 5; ++k) picks.push_back(u.first_region[c] + PER + k);
    picks.push_back(u.first_region[6] + PER + 4);
    while (picks.size() < 2190) { const int c = rnd_below(B); picks.push_back(u.first_region[c] + rnd_below(PER)); }
    for (size_t i = picks.size() - 1; i > 0; --i) std::swap(picks[i], picks[(size_t)rnd_below((int)i + 1)]);
    const int M = (int)picks.size();
    std::vector<int> first(B, 1 << 30);
    for (int i = M - 1; i >= 0; --i) first[u.sp_cloud[picks[i]]] = i;
    size_t max_region = 5000;

    for (int mode = 0; mode < 2; ++mode) {
        const int64_t budgets[2] = {700, 1 << 20};         // (ends inside the walk; everything — the dominant mode once)
        for (int64_t budget0 : budgets) {
            if (mode == 0 && budget0 != 700) continue;
            // ---- the one-call chain over the union
            std::vector<float> mask(n, 0.f), label(n, 0.f);
            std::vector<uint8_t> used(M, 7), labeled(S, 0);
            std::vector<int32_t> cls((size_t)M * 32, -5), proc(M, -1), n_items{M};
            std::vector<int64_t> out(12, -9), budget{budget0};
            CHECK(ssdr_oracle_label_dev(u.gt.data(), u.pred.data(), n, u.sp_off.data(), u.sp_pts.data(), S, u.sp_cloud.data(), B, picks.data(), n_items.data(), M, nullptr,
                                        max_region, NL, NC, mode, 0.8, 4, budget.data(), mask.data(), label.data(), used.data(), labeled.data(), cls.data(), cls.size(),
                                        proc.data(), out.data(), nullptr) == SSDR_OK);
            // ---- three ranks: contiguous shares of four clouds, their own arrays with local ids
            std::vector<uint8_t> records((size_t)W * MAXI * SSDR_LABEL_RECORD_BYTES, 0xAB);
            struct Rank { std::vector<int32_t> gt, pred, off, pts, items, n_items; std::vector<uint64_t> keys; std::vector<int> pick_of; int s0, p0; };
            std::vector<Rank> ranks(W);
            for (int r = 0; r < W; ++r) {
                Rank& R = ranks[r];
                const int c0 = r * 4, c1 = c0 + 4;
                R.s0 = u.first_region[c0]; R.p0 = u.first_point[c0];
                const int s1 = u.first_region[c1], p1 = u.first_point[c1];
                R.gt.assign(u.gt.begin() + R.p0, u.gt.begin() + p1); R.pred.assign(u.pred.begin() + R.p0, u.pred.begin() + p1);
                for (int s = R.s0; s <= s1; ++s) R.off.push_back(u.sp_off[s] - u.sp_off[R.s0]);
                for (int i = u.sp_off[R.s0]; i < u.sp_off[s1]; ++i) R.pts.push_back(u.sp_pts[i] - R.p0);
                for (int i = 0; i < M; ++i) {
                    const int c = u.sp_cloud[picks[i]];
                    if (c < c0 || c >= c1) continue;
                    R.items.push_back(picks[i] - R.s0); R.keys.push_back(((uint64_t)first[c] << 32) | (uint64_t)i); R.pick_of.push_back(i);
                }
                R.n_items.assign(1, (int32_t)R.items.size());
                CHECK((int)R.items.size() < MAXI);
                R.items.resize(MAXI, 0); R.keys.resize(MAXI, 0);
                CHECK(ssdr_oracle_label_verdict_dev(R.gt.data(), R.pred.data(), R.gt.size(), R.off.data(), R.pts.data(), R.off.size() - 1, R.items.data(), R.n_items.data(), MAXI,
                                                    R.keys.data(), max_region, NL, NC, mode, 0.8, 4, records.data() + (size_t)r * MAXI * SSDR_LABEL_RECORD_BYTES, nullptr) == SSDR_OK);
            }
            std::vector<int> walk_of(M, -1);
            int reached = 0;
            for (int r = 0; r < W; ++r) {
                Rank& R = ranks[r];
                const size_t nr = R.gt.size(), Sr = R.off.size() - 1;
                std::vector<float> rmask(nr, 0.f), rlabel(nr, 0.f);
                std::vector<uint8_t> rused(MAXI, 7), rlabeled(Sr, 0);
                std::vector<int32_t> rcls(cls.size(), -5), rpos(MAXI, -7);
                std::vector<int64_t> rout(12, -9), rbudget{budget0};
                CHECK(ssdr_oracle_label_walk_dev(records.data(), r, W, R.pred.data(), nr, R.off.data(), R.pts.data(), Sr, R.items.data(), R.n_items.data(), MAXI, max_region, NC,
                                                 rbudget.data(), rmask.data(), rlabel.data(), rused.data(), rlabeled.data(), rcls.data(), rcls.size(), rpos.data(), rout.data(),
                                                 nullptr) == SSDR_OK);
                CHECK(rout == out && rbudget == budget && rcls == cls);
                CHECK(std::memcmp(rmask.data(), mask.data() + R.p0, 4 * nr) == 0 && std::memcmp(rlabel.data(), label.data() + R.p0, 4 * nr) == 0);
                CHECK(std::memcmp(rlabeled.data(), labeled.data() + R.s0, Sr) == 0);
                for (int k = 0; k < MAXI; ++k) {
                    if (k >= R.n_items[0]) { CHECK(rused[k] == 0 && rpos[k] == -1); continue; }
                    CHECK(rused[k] == used[R.pick_of[k]]);
                    if (rpos[k] >= 0) { CHECK(rpos[k] < M && proc[rpos[k]] == R.pick_of[k]); walk_of[R.pick_of[k]] = rpos[k]; ++reached; }
                    else CHECK(rused[k] == 0);
                }
            }
            for (int j = 0; j < reached; ++j) CHECK(walk_of[proc[j]] == j);      // the walk reaches a prefix of the order
            CHECK(budget0 != 0 || reached == 0);
            CHECK(budget0 < (1 << 20) || reached == M);
            std::printf("mode %d budget %lld: %lld used, budget left %lld, %d of %d reached\n", mode, (long long)budget0, (long long)out[9], (long long)out[7], reached, M);
        }
    }
    std::printf("label halves ok\n");
    return 0;
}
