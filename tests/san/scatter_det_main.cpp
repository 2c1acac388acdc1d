// TEST INFRASTRUCTURE ONLY — a stand-alone program for the AddressSanitizer / UBSan objects of the CPU logic build (make scatter-det-san): the list
// builder and the two atomic-free reductions of csrc/scatter_det.hip through ssdr_scatter_add_rows_dev and ssdr_pool_grad_rows_dev alone.
// In the CPU logic build device memory is host memory: every array is a std::vector of exactly the size the entry is promised (a strided view ends
// with its last row's last column), so an access one element off is a report.  Results are compared bit for bit with a sequential restatement.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/ssdr_al.h"

namespace {
uint64_t g_state = 0x2545f4914f6cdd1dull;
uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }
int rnd_below(int n) { return (int)(rnd() % (uint32_t)n); }
float rnd_float() { return (float)((int)(rnd() % 20001u) - 10000) * (1.f / 4096.f); }
int clampi(int j, int n) { return j < 0 ? 0 : (j >= n ? n - 1 : j); }

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, ssdr_last_error()); return 1; } \
    } while (0)

// a view of `rows` rows of C columns, leading dimension ld, starting at column col of its buffer: the buffer ends with the view's last element
struct Strided {
    std::vector<float> buf; int ld, col, C;
    Strided(int rows, int ld_, int col_, int C_) : buf(rows > 0 ? (size_t)(rows - 1) * ld_ + col_ + C_ : 0), ld(ld_), col(col_), C(C_) { for (float& v : buf) v = rnd_float(); }
    float* p() { return buf.data() + col; }
    float& at(long r, int c) { return buf[(size_t)r * ld + col + c]; }
};

int rows_case(int B, int rows_per_b, int src_rows, int C, int ldo, int o_col, int lds, int s_col, int hub_every) {
    std::vector<int32_t> idx((size_t)B * rows_per_b);
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = hub_every && (int)(i % hub_every) == 0 ? src_rows - 1 : rnd_below(src_rows + 4) - 2;      // -2 .. src_rows + 1: clamped
    Strided dout(B * rows_per_b, ldo, o_col, C), dsrc(B * src_rows, lds, s_col, C);
    std::vector<float> want = dsrc.buf;
    {
        std::vector<float> sum((size_t)B * src_rows * C, 0.f); std::vector<char> hit((size_t)B * src_rows, 0);
        for (int b = 0; b < B; ++b) for (int r = 0; r < rows_per_b; ++r) {           // ascending r per row is ascending r overall
            const long q = (long)b * src_rows + clampi(idx[(size_t)b * rows_per_b + r], src_rows);
            hit[q] = 1;
            for (int c = 0; c < C; ++c) sum[q * C + c] = sum[q * C + c] + dout.at((long)b * rows_per_b + r, c);
        }
        for (long q = 0; q < (long)B * src_rows; ++q) if (hit[q]) for (int c = 0; c < C; ++c) want[(size_t)q * lds + s_col + c] = want[(size_t)q * lds + s_col + c] + sum[q * C + c];
    }
    CHECK(ssdr_scatter_add_rows_dev(idx.data(), B, rows_per_b, src_rows, dout.p(), ldo, C, dsrc.p(), lds, nullptr) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    CHECK(std::memcmp(want.data(), dsrc.buf.data(), 4 * want.size()) == 0);
    std::printf("rows B %d rows_per_b %d src_rows %d C %d ldo %d lds %d: ok\n", B, rows_per_b, src_rows, C, ldo, lds);
    return 0;
}

int pool_case(int B, int m_per_b, int src_rows, int C, int ldo, int o_col, int lds, int s_col) {
    std::vector<int32_t> idx((size_t)B * m_per_b * 16);
    for (int32_t& v : idx) v = rnd_below(src_rows + 2) - 1;
    for (size_t m = 0; m < idx.size() / 16; m += 3) idx[m * 16 + 5] = idx[m * 16 + 11];                  // a repeated index inside a point's 16
    Strided src(B * src_rows, lds, s_col, C), dsrc(B * src_rows, lds, s_col, C), out(B * m_per_b, ldo, o_col, C), dout(B * m_per_b, ldo, o_col, C);
    for (int b = 0; b < B; ++b) for (int j = 1; j < src_rows; j += 2) for (int c = 0; c < C; ++c) src.at((long)b * src_rows + j, c) = src.at((long)b * src_rows + j - 1, c);   // exact copies: ties
    std::vector<float> want = dsrc.buf;
    std::vector<float> sum((size_t)B * src_rows * C, 0.f); std::vector<char> hit((size_t)B * src_rows, 0);
    long tied_points = 0;
    for (int b = 0; b < B; ++b) for (int m = 0; m < m_per_b; ++m) {
        const long gm = (long)b * m_per_b + m;
        for (int c = 0; c < C; ++c) {
            float mx = 0.f; int ties = 0;
            for (int k = 0; k < 16; ++k) { const float v = src.at((long)b * src_rows + clampi(idx[gm * 16 + k], src_rows), c); mx = k == 0 || v > mx ? v : mx; }
            out.at(gm, c) = mx;
            for (int k = 0; k < 16; ++k) ties += src.at((long)b * src_rows + clampi(idx[gm * 16 + k], src_rows), c) == mx;
            tied_points += ties > 1;
            const float share = dout.at(gm, c) / (float)ties;
            for (int k = 0; k < 16; ++k) {
                const long q = (long)b * src_rows + clampi(idx[gm * 16 + k], src_rows);
                hit[q] = 1;
                if (src.at(q, c) == mx) sum[q * C + c] = sum[q * C + c] + share;
            }
        }
    }
    CHECK(tied_points > 0);
    for (long q = 0; q < (long)B * src_rows; ++q) if (hit[q]) for (int c = 0; c < C; ++c) want[(size_t)q * lds + s_col + c] = want[(size_t)q * lds + s_col + c] + sum[q * C + c];
    CHECK(ssdr_pool_grad_rows_dev(src.p(), dsrc.p(), lds, src_rows, idx.data(), B, m_per_b, C, out.p(), dout.p(), ldo, nullptr) == SSDR_OK);
    CHECK(ssdr_stream_sync(nullptr) == SSDR_OK);
    CHECK(std::memcmp(want.data(), dsrc.buf.data(), 4 * want.size()) == 0);
    std::printf("pool B %d m_per_b %d src_rows %d C %d ldo %d lds %d: ok (%ld tied maxima)\n", B, m_per_b, src_rows, C, ldo, lds, tied_points);
    return 0;
}
}  // namespace

int main() {
    CHECK(ssdr_init(0) == SSDR_OK);
    if (rows_case(1, 37, 1, 3, 3, 0, 3, 0, 0)) return 1;                // one row takes every position
    if (rows_case(3, 160, 40, 8, 11, 2, 24, 5, 0)) return 1;           // strided views on both sides
    if (rows_case(1, 9600, 600, 5, 5, 0, 5, 0, 2)) return 1;           // half of the positions on the last row: a list longer than a sort tile (2 048)
    if (rows_case(2, 512, 128, 32, 64, 0, 64, 32, 0)) return 1;        // nearest_interpolation's shape
    if (rows_case(1, 128, 8, 1024, 1024, 0, 1024, 0, 0)) return 1;     // wide and short
    if (rows_case(2, 2048, 7, 2, 3, 1, 4, 1, 0)) return 1;             // exactly two sort tiles
    if (pool_case(1, 20, 64, 5, 5, 0, 5, 0)) return 1;
    if (pool_case(2, 9, 33, 5, 7, 1, 8, 2)) return 1;                  // the second tile's offsets, strided views
    if (pool_case(3, 300, 40, 16, 16, 0, 16, 0)) return 1;             // 14 400 positions: several sort tiles
    {   // nothing to do: no launch, no access
        std::vector<int32_t> idx(1); std::vector<float> a(1), b(1);
        CHECK(ssdr_scatter_add_rows_dev(idx.data(), 0, 5, 3, a.data(), 1, 1, b.data(), 1, nullptr) == SSDR_OK);
        CHECK(ssdr_scatter_add_rows_dev(idx.data(), 1, 1, 1, a.data(), 1, 0, b.data(), 1, nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_scatter_add_rows_dev(idx.data(), 1, 1, 1, a.data(), 1, 2, b.data(), 2, nullptr) == SSDR_ERR_INVALID);
        CHECK(ssdr_pool_grad_rows_dev(a.data(), b.data(), 1, 1, nullptr, 1, 1, 1, a.data(), a.data(), 1, nullptr) == SSDR_ERR_INVALID);
    }
    std::printf("scatter det ok\n");
    return 0;
}
