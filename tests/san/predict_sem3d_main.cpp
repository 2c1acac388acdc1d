// TEST INFRASTRUCTURE ONLY — a stand-alone program for the AddressSanitizer / UBSan objects of the CPU logic build (make predict-sem3d-san): the three
// entries of the Semantic3D prediction pass in csrc/predict.hip, ssdr_predict_scan_tile_dev, ssdr_predict_parts_dev and ssdr_predict_scatter_dev.
// In the CPU logic build device memory is host memory: every array is a std::vector of exactly the size the entry is promised, so an access one
// element off is a report.  Results are compared with a plain restatement.  Run it with ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0
// (the CPU build keeps its fibre stacks for the life of its worker threads).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>
#include "../../include/ssdr_al.h"

namespace {
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, ssdr_last_error()); return 1; } \
    } while (0)

int run(int n0, int n1) {
    std::mt19937 gen(7);
    std::uniform_real_distribution<float> u(0.f, 4.f);
    const int sizes[2] = {n0, n1}, base[2] = {0, n0}, n = n0 + n1;
    std::vector<float> pts(3 * n), col(3 * n);
    for (auto& v : pts) v = u(gen);
    for (auto& v : col) v = u(gen) * 0.25f;
    for (int i = 0; i < 3 * 40; ++i) pts[3 * (n0 - 40) + i] = pts[i];                 // duplicates: tie rows
    std::vector<int32_t> labels(n), perm(n);
    for (auto& v : labels) v = (int32_t)(gen() % 8);
    std::vector<float> t_xyz(3 * n, -1.f), t_feat(6 * n, -1.f);
    std::vector<int32_t> t_idx(n, -1);
    const float scale = 0.5f;
    float centers[2][3];
    for (int c = 0; c < 2; ++c) {
        const int o = base[c], m = sizes[c];
        std::iota(perm.begin() + o, perm.begin() + o + m, 0);
        std::shuffle(perm.begin() + o, perm.begin() + o + m, gen);
        for (int k = 0; k < 3; ++k) centers[c][k] = pts[3 * (o + 5) + k] + 0.1f * (k + 1);
        CHECK(ssdr_predict_scan_tile_dev(pts.data() + 3 * o, col.data() + 3 * o, m, centers[c], perm.data() + o, scale, t_xyz.data() + 3 * o,
                                         t_feat.data() + 6 * o, t_idx.data() + o, nullptr) == SSDR_OK);
    }
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    for (int c = 0; c < 2; ++c) {                                                      // tile.hip's rule with num_points = n, restated
        const int o = base[c], m = sizes[c];
        const float* P = pts.data() + 3 * o; const float* ce = centers[c];
        std::vector<float> d(m);
        for (int i = 0; i < m; ++i) { const float x = P[3 * i] - ce[0], y = P[3 * i + 1] - ce[1], z = P[3 * i + 2] - ce[2]; d[i] = (x * x + y * y) + z * z; }
        std::vector<int> order(m);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return d[a] < d[b]; });
        for (int r = 0; r < m; ++r) {
            const int id = order[perm[o + r]];
            CHECK(t_idx[o + r] == id);
            for (int k = 0; k < 3; ++k) {
                CHECK(t_xyz[3 * (o + r) + k] == P[3 * id + k] - ce[k]);
                CHECK(t_feat[6 * (o + r) + k] == P[3 * id + k] - ce[k]);
                CHECK(t_feat[6 * (o + r) + 3 + k] == col[3 * (o + id) + k] * scale);
            }
        }
    }
    // parts: each scan cut in two at an odd row, its rows dealt out alternately (ascending inside a part, as ssdr_split3_dev leaves them)
    std::vector<int32_t> order(n);
    std::vector<int64_t> off{0}, pbase;
    for (int c = 0; c < 2; ++c) {
        const int o = base[c], m = sizes[c];
        int at = o;
        for (int half = 0; half < 2; ++half) {
            for (int r = half; r < m; r += 2) order[at++] = r;
            off.push_back(at); pbase.push_back(o);
        }
    }
    const int32_t ratios[2] = {4, 4};
    const size_t np = 4;
    int64_t P[3];
    std::vector<int64_t> rel(off);
    CHECK(ssdr_predict_layout(rel.data(), np, 1, 2, ratios, P) == SSDR_OK);
    CHECK(P[0] == n);
    std::vector<float> cm_xyz(3 * n, -1.f), pk_xyz(3 * n, -1.f), pk_feat(6 * n, -1.f);
    std::vector<int32_t> pk_src(n, -1), pk_lab(n, -1);
    // two calls, as two chunks: parts [0, 3) and part 3 alone (absolute offsets, the second chunk's first offset is not 0)
    const size_t first = 3;
    const int64_t rows0 = off[first];
    CHECK(ssdr_predict_parts_dev(t_xyz.data(), t_feat.data(), t_idx.data(), labels.data(), order.data(), off.data(), pbase.data(), first, 2, ratios,
                                 cm_xyz.data(), pk_xyz.data(), pk_feat.data(), pk_src.data(), pk_lab.data(), nullptr) == SSDR_OK);
    CHECK(ssdr_predict_parts_dev(t_xyz.data(), t_feat.data(), t_idx.data(), labels.data(), order.data(), off.data() + first, pbase.data() + first, np - first, 2,
                                 ratios, cm_xyz.data() + 3 * rows0, pk_xyz.data() + 3 * rows0, pk_feat.data() + 6 * rows0, pk_src.data() + rows0,
                                 pk_lab.data() + rows0, nullptr) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    std::vector<int> seen(n, 0);
    for (int q = 0; q < n; ++q) {
        int k = 0;
        while (off[k + 1] <= q) ++k;
        const int64_t row = pbase[k] + order[q];
        for (int j = 0; j < 3; ++j) CHECK(cm_xyz[3 * q + j] == t_xyz[3 * row + j]);
    }
    for (int p = 0; p < n; ++p) {                                                      // every packed row holds one tile row, whole
        const int src = pk_src[p];
        CHECK(src >= 0 && src < n && pk_lab[p] == labels[src]);
        ++seen[src];
    }
    for (int i = 0; i < n; ++i) CHECK(seen[i] == 1);
    // read-back: coded rows, one of them with a source outside the output
    const int C = 13;
    std::vector<float> pp((size_t)n * C), pf((size_t)n * 32), probs((size_t)n * C, -7.f), feat((size_t)n * 32, -7.f);
    for (size_t i = 0; i < pp.size(); ++i) pp[i] = (float)i / 7;
    for (size_t i = 0; i < pf.size(); ++i) pf[i] = -(float)i / 3;
    std::vector<int32_t> src(pk_src);
    const int lost = src[n - 1];
    src[n - 1] = n;
    CHECK(ssdr_predict_scatter_dev(src.data(), n, pp.data(), C, pf.data(), n, probs.data(), feat.data(), nullptr) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    for (int r = 0; r < n - 1; ++r) {
        CHECK(std::memcmp(&probs[(size_t)src[r] * C], &pp[(size_t)r * C], 4 * C) == 0);
        CHECK(std::memcmp(&feat[(size_t)src[r] * 32], &pf[(size_t)r * 32], 128) == 0);
    }
    CHECK(probs[(size_t)lost * C] == -7.f && feat[(size_t)lost * 32 + 31] == -7.f);
    std::printf("scans of %d and %d points: tile, parts and read-back ok\n", n0, n1);
    return 0;
}
}  // namespace

int main() {
    if (ssdr_init(0) != SSDR_OK) { std::printf("ssdr_init failed: %s\n", ssdr_last_error()); return 1; }
    if (run(301, 1029) || run(2048, 257)) return 1;
    std::printf("ok\n");
    return 0;
}
