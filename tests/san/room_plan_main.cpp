// TEST INFRASTRUCTURE ONLY — a stand-alone program for the AddressSanitizer / UBSan objects of the CPU logic build (make room-plan-san): the lifetime of a
// room plan (csrc/frontend.hip: FePlan) through ssdr_rooms_plan_create_dev, ssdr_tile_from_rooms_planned_batch_dev and ssdr_rooms_plan_destroy alone.
// In the CPU logic build device memory is host memory: every input and output is a std::vector of exactly the size the entry is promised, so an access one
// element off is a report, and so is a planned call that reads a plan after its destruction.  Every planned call is compared with ssdr_tile_from_rooms_batch_dev on
// the same inputs, byte for byte.  Run it as tests/test_frontend_room_plan.py does, with ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0: the CPU build
// keeps its fibre stacks for the life of its worker threads.
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

uint32_t g_state = 12345u;
float unit() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) * (1.0f / 16777216.0f); }

struct Rooms {
    size_t R, N, fdim, ldim; std::vector<int64_t> off; std::vector<float> p, f; std::vector<int32_t> c, perm; std::vector<float> dup;
    size_t nt() const { return (size_t)off[R]; }
};
struct Out {
    std::vector<float> sub_p, sub_f, xyz, feat; std::vector<int32_t> sub_c, lab; std::vector<int64_t> m; std::vector<int32_t> stage, reduced, buckets; int32_t status;
    explicit Out(const Rooms& r)
        : sub_p(3 * r.nt(), -7.f), sub_f(r.fdim * r.nt(), -7.f), xyz(3 * r.R * r.N, -7.f), feat((3 + r.fdim) * r.R * r.N, -7.f), sub_c(r.ldim * r.nt(), -7), lab(r.R * r.N, -7),
          m(r.R, -7), stage(r.R, -7), reduced(r.R, -7), buckets(r.R, -7), status(-7) {}
    bool same(const Out& o) const {
        return sub_p == o.sub_p && sub_f == o.sub_f && xyz == o.xyz && feat == o.feat && sub_c == o.sub_c && lab == o.lab && m == o.m && stage == o.stage && reduced == o.reduced &&
               buckets == o.buckets && status == o.status;
    }
};

Rooms make_rooms(const std::vector<size_t>& sizes, size_t N, size_t fdim, size_t ldim) {
    Rooms r; r.R = sizes.size(); r.N = N; r.fdim = fdim; r.ldim = ldim; r.off.assign(1, 0);
    for (size_t k = 0; k < sizes.size(); ++k) {
        const float ext[3] = {2.0f + (float)k, 1.5f, 1.2f}, shift = 5.f * (float)k;
        for (size_t i = 0; i < sizes[k]; ++i) {
            for (int d = 0; d < 3; ++d) r.p.push_back(unit() * ext[d] + (d == 0 ? shift : 0.f));
            for (size_t q = 0; q < fdim; ++q) r.f.push_back((float)(int)(unit() * 256.f));
            for (size_t q = 0; q < ldim; ++q) r.c.push_back((int32_t)(unit() * 13.f));
        }
        r.off.push_back(r.off.back() + (int64_t)sizes[k]);
    }
    for (size_t k = 0; k < r.R; ++k) for (size_t i = 0; i < N; ++i) { r.perm.push_back((int32_t)((i * 7 + k) % N)); r.dup.push_back(i + 1 == N ? 1.f : unit()); }      // (7 and N = 2^k: a permutation)
    return r;
}

int call(const Rooms& r, const void* plan, const float* centres, float dl, const int64_t* off, size_t R, void* stream, Out& o) {
    const float* f = r.fdim ? r.f.data() : nullptr; const int32_t* c = r.ldim ? r.c.data() : nullptr;
    float* of = r.fdim ? o.sub_f.data() : nullptr; int32_t* oc = r.ldim ? o.sub_c.data() : nullptr; int32_t* ol = r.ldim == 1 ? o.lab.data() : nullptr;
    if (plan) return ssdr_tile_from_rooms_planned_batch_dev(plan, r.p.data(), f, r.fdim, c, r.ldim, off, R, dl, o.sub_p.data(), of, oc, o.m.data(), centres, r.N, r.perm.data(),
                                                            r.dup.data(), 1.f / 255.f, o.xyz.data(), o.feat.data(), nullptr, ol, stream);
    return ssdr_tile_from_rooms_batch_dev(r.p.data(), f, r.fdim, c, r.ldim, off, R, dl, o.sub_p.data(), of, oc, o.m.data(), centres, r.N, r.perm.data(), r.dup.data(), 1.f / 255.f,
                                          o.xyz.data(), o.feat.data(), nullptr, ol, stream);
}
int finish(const Rooms& r, void* stream, Out& o) {
    (void)ssdr_grid_subsample_status(stream, &o.status);
    return ssdr_tile_from_rooms_stats(stream, o.stage.data(), o.reduced.data(), o.buckets.data(), r.R);
}

int lifetime_case(size_t fdim, size_t ldim) {
    const float dl = 0.04f;
    const Rooms r = make_rooms({3000, 33000}, 256, fdim, ldim);          // 33000: two chunks of the count / scatter kernels
    const std::vector<float> cen1 = {1.0f, 0.7f, 0.6f, 6.5f, 0.2f, 1.1f};
    void *plan = nullptr, *s1 = nullptr, *s2 = nullptr;
    CHECK(ssdr_stream_create(&s1) == SSDR_OK && ssdr_stream_create(&s2) == SSDR_OK);
    CHECK(ssdr_rooms_plan_create_dev(r.p.data(), r.fdim ? r.f.data() : nullptr, r.fdim, r.ldim ? r.c.data() : nullptr, r.ldim, r.off.data(), r.R, dl, s1, &plan) == SSDR_OK && plan);
    {   // built on s1, first used on s2
        Out ref(r), got(r);
        CHECK(call(r, nullptr, cen1.data(), dl, r.off.data(), r.R, nullptr, ref) == SSDR_OK && finish(r, nullptr, ref) == SSDR_OK);
        CHECK(call(r, plan, cen1.data(), dl, r.off.data(), r.R, s2, got) == SSDR_OK && finish(r, s2, got) == SSDR_OK);
        CHECK(ref.m[0] > 0 && ref.stage[0] >= 1);
        CHECK(got.same(ref));
    }
    {   // a plan answers for its own inputs only: nothing is launched, nothing written
        Out o(r); const Out untouched(r);
        std::vector<int64_t> moved = r.off; moved[1] += 3;
        CHECK(call(r, plan, cen1.data(), 0.05f, r.off.data(), r.R, nullptr, o) == SSDR_ERR_INVALID);
        CHECK(call(r, plan, cen1.data(), dl, moved.data(), r.R, nullptr, o) == SSDR_ERR_INVALID);
        CHECK(call(r, plan, cen1.data(), dl, r.off.data(), r.R - 1, nullptr, o) == SSDR_ERR_INVALID);
        CHECK(std::strstr(ssdr_last_error(), "plan") != nullptr);
        CHECK(o.sub_p == untouched.sub_p && o.xyz == untouched.xyz && o.m == untouched.m);
    }
    CHECK(ssdr_rooms_plan_destroy(plan) == SSDR_OK);
    CHECK(ssdr_rooms_plan_destroy(nullptr) == SSDR_OK);
    {   // new points behind the same pointers, a new plan: the planned call follows them
        Rooms q = r;
        for (size_t i = 0; i < q.p.size(); ++i) q.p[i] = r.p[i] * 0.75f + 0.01f;
        void* plan2 = nullptr;
        CHECK(ssdr_rooms_plan_create_dev(q.p.data(), q.fdim ? q.f.data() : nullptr, q.fdim, q.ldim ? q.c.data() : nullptr, q.ldim, q.off.data(), q.R, dl, nullptr, &plan2) == SSDR_OK);
        Out ref(q), got(q);
        CHECK(call(q, nullptr, cen1.data(), dl, q.off.data(), q.R, s1, ref) == SSDR_OK && finish(q, s1, ref) == SSDR_OK);
        CHECK(call(q, plan2, cen1.data(), dl, q.off.data(), q.R, s1, got) == SSDR_OK && finish(q, s1, got) == SSDR_OK);
        CHECK(got.same(ref));
        CHECK(ssdr_rooms_plan_destroy(plan2) == SSDR_OK);
    }
    CHECK(ssdr_stream_destroy(s1) == SSDR_OK && ssdr_stream_destroy(s2) == SSDR_OK);
    std::printf("lifetime, rows of 3 + %zu + %zu words: ok\n", fdim, ldim);
    return 0;
}
}  // namespace

int main() {
    if (ssdr_init(0) != SSDR_OK) { std::printf("init failed: %s\n", ssdr_last_error()); return 1; }
    if (lifetime_case(3, 1)) return 1;
    {   // arguments a plan cannot be built from
        void* plan = reinterpret_cast<void*>(1);
        std::vector<float> p(30, 0.5f); const int64_t off[2] = {0, 10}, empty[2] = {0, 0};
        if (ssdr_rooms_plan_create_dev(p.data(), nullptr, 0, nullptr, 0, off, 1, 0.f, nullptr, &plan) != SSDR_ERR_INVALID || plan) { std::printf("FAILED: dl 0\n"); return 1; }
        if (ssdr_rooms_plan_create_dev(p.data(), nullptr, 0, nullptr, 0, empty, 1, 0.04f, nullptr, &plan) != SSDR_ERR_EMPTY || plan) { std::printf("FAILED: empty cloud\n"); return 1; }
        if (ssdr_rooms_plan_create_dev(p.data(), p.data(), 5, nullptr, 0, off, 1, 0.04f, nullptr, &plan) != SSDR_ERR_UNSUPPORTED || plan) { std::printf("FAILED: wide rows\n"); return 1; }
    }
    std::printf("room plan ok\n");
    return 0;
}
