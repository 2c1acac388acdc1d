// TEST INFRASTRUCTURE ONLY — a stand-alone program for the AddressSanitizer / UBSan objects of the CPU logic build (make train-exchange-san): the
// kernels of csrc/train_exchange.hip on either side of a data-parallel step's collectives: the two packs, the two merges (through
// ssdr_bn_stats_merge_dev and ssdr_rank_sums_merge_dev) and the range-table zeroing, at world 3.
// In the CPU logic build device memory is host memory: every array is a std::vector of exactly the size the kernel is promised, so an access one
// element off is a report.  Results are compared bit for bit with scalar loops.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "train_exchange.hpp"

namespace {
uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }
float rnd_float() { return (float)((int)(rnd() % 20001u) - 10000) * (1.f / 4096.f); }

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, ssdr_last_error()); return 1; } \
    } while (0)

bool same(const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), 4 * a.size()) == 0); }

constexpr int WORLD = 3;

// the chunks of M rows -> the record, as pack_stats_kernel
int pack_stats_case(int M, int chunk, int C) {
    const int nchunks = (M + chunk - 1) / chunk;
    std::vector<float> part((size_t)nchunks * 2 * C), rec(1 + 2 * (size_t)C, -1.f), want(rec.size());
    for (int k = 0; k < nchunks; ++k) for (int c = 0; c < C; ++c) { part[((size_t)k * 2) * C + c] = 100.f + rnd_float(); part[((size_t)k * 2 + 1) * C + c] = std::fabs(rnd_float()) * 10.f; }
    want[0] = (float)M;
    for (int c = 0; c < C; ++c) {
        float n = 0.f, mu = 0.f, m2 = 0.f;
        for (int k = 0; k < nchunks; ++k) {
            const float nb = (float)(std::min(M, (k + 1) * chunk) - k * chunk), d = part[((size_t)k * 2) * C + c] - mu, nn = n + nb;
            mu += d * (nb / nn); m2 += part[((size_t)k * 2 + 1) * C + c] + d * d * (n * nb / nn); n = nn;
        }
        want[1 + c] = mu; want[1 + C + c] = m2;
    }
    CHECK(ssdr::xchg_pack_stats(part.data(), nchunks, chunk, M, C, rec.data(), ssdr::pick_stream(nullptr)) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    CHECK(same(rec, want));
    std::printf("pack stats M %d chunk %d C %d: ok\n", M, chunk, C);
    return 0;
}

int pack_sums_case(int nchunks, int C, int swap) {
    std::vector<float> part((size_t)nchunks * 2 * C), out(2 * (size_t)C, -1.f), want(out.size());
    for (float& v : part) v = rnd_float();
    for (int c = 0; c < C; ++c) {
        float x0 = 0.f, x1 = 0.f;
        for (int k = 0; k < nchunks; ++k) { x0 += part[((size_t)k * 2) * C + c]; x1 += part[((size_t)k * 2 + 1) * C + c]; }
        want[(swap ? C : 0) + c] = x0; want[(swap ? 0 : C) + c] = x1;
    }
    CHECK(ssdr::xchg_pack_sums(part.data(), nchunks, C, out.data(), swap, ssdr::pick_stream(nullptr)) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    CHECK(same(out, want));
    std::printf("pack sums chunks %d C %d swap %d: ok\n", nchunks, C, swap);
    return 0;
}

int merge_stats_case(int C, int unbiased, bool moving) {
    const size_t stride = 1 + 2 * (size_t)C;
    const float counts[WORLD] = {3.f, 1.f, 3932160.f};
    std::vector<float> rec(WORLD * stride), mean(C, -1.f), inv(C, -1.f), cnt(1, -1.f), mm(moving ? C : 0), mv(moving ? C : 0);
    for (int r = 0; r < WORLD; ++r) {
        rec[r * stride] = counts[r];
        for (int c = 0; c < C; ++c) { rec[r * stride + 1 + c] = (c % 2 ? 0.f : 1000.f) + rnd_float() * 0.01f; rec[r * stride + 1 + C + c] = counts[r] == 1.f ? 0.f : counts[r] * std::fabs(rnd_float()) * 0.1f; }
    }
    for (float& v : mm) v = rnd_float();
    for (float& v : mv) v = std::fabs(rnd_float()) + 0.1f;
    std::vector<float> w_mean(C), w_inv(C), w_cnt(1), w_mm = mm, w_mv = mv;
    for (int c = 0; c < C; ++c) {
        float n = 0.f, mu = 0.f, m2 = 0.f;
        for (int r = 0; r < WORLD; ++r) {
            const float nb = rec[r * stride], d = rec[r * stride + 1 + c] - mu, nn = n + nb;
            mu += d * (nb / nn); m2 += rec[r * stride + 1 + C + c] + d * d * (n * nb / nn); n = nn;
        }
        const float var = m2 / n;
        w_mean[c] = mu; w_inv[c] = 1.f / std::sqrt(var + 1e-6f); w_cnt[0] = n;
        if (moving) {
            const float vm = (unbiased && n > 1.f) ? var * (n / (n - 1.f)) : var;
            w_mm[c] -= (w_mm[c] - mu) * (1.f - 0.99f); w_mv[c] -= (w_mv[c] - vm) * (1.f - 0.99f);
        }
    }
    CHECK(ssdr_bn_stats_merge_dev(rec.data(), WORLD, C, mean.data(), inv.data(), cnt.data(), moving ? mm.data() : nullptr, moving ? mv.data() : nullptr, unbiased, nullptr) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    CHECK(same(mean, w_mean) && same(inv, w_inv) && same(cnt, w_cnt) && same(mm, w_mm) && same(mv, w_mv));
    CHECK(cnt[0] == 3932164.f);
    std::printf("merge stats C %d unbiased %d moving %d: ok\n", C, unbiased, (int)moving);
    return 0;
}

int merge_sums_case(int n) {
    std::vector<float> rec((size_t)WORLD * n), out(n, -1.f), want(n);
    for (float& v : rec) v = rnd_float();
    for (int r = 0; r < WORLD; ++r) rec[(size_t)r * n] = -0.f;
    for (int i = 0; i < n; ++i) { float x = 0.f; for (int r = 0; r < WORLD; ++r) x += rec[(size_t)r * n + i]; want[i] = x; }
    CHECK(ssdr_rank_sums_merge_dev(rec.data(), WORLD, n, out.data(), nullptr) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    CHECK(same(out, want) && !std::signbit(out[0]));
    std::printf("merge sums n %d: ok\n", n);
    return 0;
}

// ranges of 2 C floats behind weights of varying size, the last one ending with the array
int zero_ranges_case() {
    const int widths[] = {8, 1, 65, 1024, 63};
    std::vector<long> table; long at = 0;
    for (int w : widths) { at += 3L * w + 1; table.push_back(at); table.push_back(2L * w); at += 2L * w; }
    std::vector<float> g((size_t)at), want;
    for (float& v : g) v = 1.f + std::fabs(rnd_float());
    want = g;
    for (size_t i = 0; i < table.size(); i += 2) for (long e = 0; e < table[i + 1]; ++e) want[(size_t)(table[i] + e)] = 0.f;
    CHECK(ssdr::xchg_zero_ranges(g.data(), table.data(), (int)(table.size() / 2), ssdr::pick_stream(nullptr)) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    CHECK(same(g, want) && g.back() == 0.f && g[0] != 0.f);
    CHECK(ssdr::xchg_zero_ranges(g.data(), table.data(), 0, ssdr::pick_stream(nullptr)) == SSDR_OK);
    std::printf("zero ranges: ok\n");
    return 0;
}
}  // namespace

int main() {
    CHECK(ssdr_init(0) == SSDR_OK);
    if (pack_stats_case(1, 1, 1)) return 1;
    if (pack_stats_case(1000, 333, 63)) return 1;             // a short last chunk
    if (pack_stats_case(4096, 256, 65)) return 1;
    if (pack_stats_case(37, 64, 1024)) return 1;              // one chunk, the widest unit
    for (int swap = 0; swap < 2; ++swap) { if (pack_sums_case(1, 1, swap)) return 1; if (pack_sums_case(7, 64, swap)) return 1; if (pack_sums_case(3, 1024, swap)) return 1; if (pack_sums_case(5, 65, swap)) return 1; }
    for (int C : {1, 8, 63, 64, 65, 1024}) for (int unbiased = 0; unbiased < 2; ++unbiased) { if (merge_stats_case(C, unbiased, false)) return 1; if (merge_stats_case(C, unbiased, true)) return 1; }
    for (int n : {1, 3, 64, 65, 2048}) if (merge_sums_case(n)) return 1;
    if (zero_ranges_case()) return 1;
    {   // refused before anything is read
        std::vector<float> a(1);
        CHECK(ssdr_bn_stats_merge_dev(nullptr, 1, 1, a.data(), a.data(), a.data(), nullptr, nullptr, 0, nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_bn_stats_merge_dev(a.data(), 0, 1, a.data(), a.data(), a.data(), nullptr, nullptr, 0, nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_bn_stats_merge_dev(a.data(), 1, 0, a.data(), a.data(), a.data(), nullptr, nullptr, 0, nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_rank_sums_merge_dev(a.data(), 0, 1, a.data(), nullptr) == SSDR_ERR_INVALID);
    }
    std::printf("train exchange ok\n");
    return 0;
}
