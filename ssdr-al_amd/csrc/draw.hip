// The generators' per-row randomness, drawn on the device (include/ssdr_al.h, "per-row draws"): the shuffle permutations, the
// padding draws and Semantic3D's augmentation noise of a batch as pure functions of a counter (seed, epoch, step, kind, element), the way the
// dropout mask is a function of (seed, step, index).  The header states the chain; draw_word below is that statement in code.  Nothing here
// depends on the launch geometry: every kernel is a grid-stride loop whose body reads nothing but its own element index.
//
// Permutations: row t is the stable argsort of 32-bit hashed keys.  One kernel writes the (key, row) pairs of every tile into the sort buffers,
// the segmented radix sort (radix_sort.hip) orders all tiles in the same launches with ceil(key_bits / 8) wide passes, one kernel unpacks the
// values into the dense array.  A segment's offset must be a multiple of the 2048-pair sort tile, so a tile of N rows owns ceil(N / 2048) * 2048
// slots.  Tiles of at most 1024 rows share a segment, up to 65536 of them (8192 tiles of 64 rows would otherwise own 2048 slots each and sort
// in 128 rounds of 64 segments): the tile's rank inside its segment sits above the key bits, so the segment comes out tile by tile, every tile
// by key, ties by row, at the price of ceil(log2(tiles) / 8) more passes.
#include "ssdr_internal.hpp"
#include "draw_word.hpp"
#include <cmath>

namespace ssdr {
namespace {

// (DrawBase, draw_base and draw_word: draw_word.hpp)
// 53 hashed bits from words j and j + 1: the upper 27 of the first above the upper 26 of the second
__device__ __forceinline__ uint64_t draw_bits53(DrawBase b, uint64_t e, uint32_t j) {
    return ((uint64_t)(draw_word(b, e, j) >> 5) << 26) | (uint64_t)(draw_word(b, e, j + 1) >> 6);
}

constexpr int DRAW_BS = 256, DRAW_MAX_BLOCKS = 2048;
constexpr long PERM_PACK = 65536;
inline unsigned draw_blocks(long n) { return (unsigned)std::max(1L, std::min((n + DRAW_BS - 1) / DRAW_BS, (long)DRAW_MAX_BLOCKS)); }

// how the tiles of a permutation call lie in the sort buffers
struct PermLayout {
    long num_tiles, N;
    long per_seg;        // tiles per segment: 1, or up to PERM_PACK when N <= 1024
    long seg_slots;      // slots a segment owns (a multiple of the sort tile); its tiles lie densely from its first slot
    long nseg;
    int key_bits, sort_bits;
};

__global__ __launch_bounds__(DRAW_BS) void perm_keys_kernel(DrawBase b, uint64_t first_tile, PermLayout l, uint64_t* keys, uint32_t* vals) {
    const long total = l.num_tiles * l.N, stride = (long)gridDim.x * DRAW_BS;
    for (long i = (long)blockIdx.x * DRAW_BS + threadIdx.x; i < total; i += stride) {
        const long t = i / l.N, r = i - t * l.N, sg = t / l.per_seg, in_seg = t - sg * l.per_seg;
        const uint64_t tile = first_tile + (uint64_t)t;
        const uint32_t k = draw_word(b, (tile << 32) | (uint64_t)r, 0u) >> (32 - l.key_bits);
        const long slot = sg * l.seg_slots + in_seg * l.N + r;
        keys[slot] = ((uint64_t)in_seg << l.key_bits) | (uint64_t)k;
        vals[slot] = (uint32_t)r;
    }
}
__global__ __launch_bounds__(DRAW_BS) void perm_unpack_kernel(PermLayout l, const uint32_t* vals, int32_t* perm) {
    const long total = l.num_tiles * l.N, stride = (long)gridDim.x * DRAW_BS;
    for (long i = (long)blockIdx.x * DRAW_BS + threadIdx.x; i < total; i += stride) {
        const long t = i / l.N, r = i - t * l.N, sg = t / l.per_seg, in_seg = t - sg * l.per_seg;
        perm[i] = (int32_t)vals[sg * l.seg_slots + in_seg * l.N + r];
    }
}

__global__ __launch_bounds__(DRAW_BS) void uniform_kernel(DrawBase b, uint64_t first, long n, float* out) {
    const long stride = (long)gridDim.x * DRAW_BS;
    for (long i = (long)blockIdx.x * DRAW_BS + threadIdx.x; i < n; i += stride)
        out[i] = (float)(draw_word(b, first + (uint64_t)i, 0u) >> 8) * 0x1p-24f;          // 24 bits: exact in float32
}

__global__ __launch_bounds__(DRAW_BS) void normal_kernel(DrawBase b, uint64_t first, long n, double scale, double* out) {
    const long stride = (long)gridDim.x * DRAW_BS;
    for (long i = (long)blockIdx.x * DRAW_BS + threadIdx.x; i < n; i += stride) {
        const uint64_t e = first + (uint64_t)i;
        const double u1 = (double)(draw_bits53(b, e, 0u) + 1ull) * 0x1p-53;               // (0, 1]: 2^53 itself is exact
        const double u2 = (double)draw_bits53(b, e, 2u) * 0x1p-53;                        // [0, 1)
        const double rad = sqrt(-2.0 * log(u1));
        const double z = rad * cos(6.283185307179586 * u2);
        out[i] = scale * z;
    }
}

struct DrawScratch { DevBuf keys, vals; RadixSorter sorter; };

}  // namespace
}  // namespace ssdr

using namespace ssdr;

extern "C" {

int ssdr_draw_perm_dev(uint64_t seed, uint32_t epoch, uint32_t step, uint64_t first_tile, size_t num_tiles, size_t num_points, int key_bits,
                       int32_t* d_perm, void* stream) {
    if (!d_perm) { set_error("draw_perm: NULL pointer"); return SSDR_ERR_INVALID; }
    if (num_tiles == 0 || num_points == 0) { set_error("draw_perm: %zu tiles of %zu rows", num_tiles, num_points); return SSDR_ERR_INVALID; }
    if (key_bits < 1 || key_bits > 32) { set_error("draw_perm: key_bits = %d is outside 1 .. 32", key_bits); return SSDR_ERR_INVALID; }
    if (first_tile > 0xffffffffull || num_tiles > 0x100000000ull - first_tile) { set_error("draw_perm: tile ids must stay below 2^32"); return SSDR_ERR_INVALID; }
    if (num_points > 0x3fffffffull || num_tiles > 0x3fffffffull) { set_error("draw_perm: more than 0x3fffffff padded pairs"); return SSDR_ERR_UNSUPPORTED; }
    PermLayout l;
    l.num_tiles = (long)num_tiles; l.N = (long)num_points; l.key_bits = key_bits;
    l.per_seg = l.N <= RADIX_TILE / 2 ? std::min(l.num_tiles, PERM_PACK) : 1;
    l.seg_slots = (l.per_seg * l.N + RADIX_TILE - 1) / RADIX_TILE * RADIX_TILE;
    l.nseg = (l.num_tiles + l.per_seg - 1) / l.per_seg;
    int rank_bits = 0;
    while ((1L << rank_bits) < l.per_seg) ++rank_bits;
    l.sort_bits = key_bits + rank_bits;
    const long slots = l.nseg * l.seg_slots;            // at most 2^30 * 2^30: no overflow
    if (slots > 0x3fffffffL) { set_error("draw_perm: %ld padded pairs, more than 0x3fffffff", slots); return SSDR_ERR_UNSUPPORTED; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    DrawScratch& sc = per_stream<DrawScratch>(s);
    SSDR_TRY(sc.keys.reserve(8 * (size_t)slots)); SSDR_TRY(sc.vals.reserve(4 * (size_t)slots));
    const DrawBase b = draw_base(seed, epoch, step, SSDR_DRAW_PERM);
    uint64_t* keys = sc.keys.as<uint64_t>(); uint32_t* vals = sc.vals.as<uint32_t>();
    const long total = l.num_tiles * l.N;
    ProfScope prof("draw_perm", s, 4.0 * (double)total);          // with ssdr_prof_enable: HIP events around the whole chain, keys to unpack
    hipLaunchKernelGGL(perm_keys_kernel, dim3(draw_blocks(total)), dim3(DRAW_BS), 0, s, b, first_tile, l, keys, vals);
    SSDR_HIP(hipGetLastError());
    sc.sorter.wide_high = true;          // a shared segment carries the tile's rank above bit 32: wide passes up there too when it is large
    for (long s0 = 0; s0 < l.nseg; s0 += RADIX_MAX_SEG) {
        const int ns = (int)std::min((long)RADIX_MAX_SEG, l.nseg - s0);
        int off[RADIX_MAX_SEG + 1], cnt[RADIX_MAX_SEG];
        for (int i = 0; i <= ns; ++i) off[i] = (int)(i * l.seg_slots);
        for (int i = 0; i < ns; ++i) cnt[i] = (int)(std::min(l.per_seg, l.num_tiles - (s0 + i) * l.per_seg) * l.N);
        SSDR_TRY(sc.sorter.sort_segments(keys + s0 * l.seg_slots, vals + s0 * l.seg_slots, ns, off, cnt, nullptr, s, l.sort_bits));
    }
    hipLaunchKernelGGL(perm_unpack_kernel, dim3(draw_blocks(total)), dim3(DRAW_BS), 0, s, l, vals, d_perm);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_draw_uniform_dev(uint64_t seed, uint32_t epoch, uint32_t step, uint32_t kind, uint64_t first, size_t n, float* d_out, void* stream) {
    if (!d_out || n == 0) { set_error("draw_uniform: NULL pointer or n = 0"); return SSDR_ERR_INVALID; }
    if (n > 0x7fffffffffffffffull) { set_error("draw_uniform: n does not fit 63 bits"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    ProfScope prof("draw_uniform", s, 4.0 * (double)n);
    hipLaunchKernelGGL(uniform_kernel, dim3(draw_blocks((long)n)), dim3(DRAW_BS), 0, s, draw_base(seed, epoch, step, kind), first, (long)n, d_out);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_draw_normal_dev(uint64_t seed, uint32_t epoch, uint32_t step, uint32_t kind, uint64_t first, size_t n, double scale, double* d_out,
                         void* stream) {
    if (!d_out || n == 0) { set_error("draw_normal: NULL pointer or n = 0"); return SSDR_ERR_INVALID; }
    if (n > 0x7fffffffffffffffull) { set_error("draw_normal: n does not fit 63 bits"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    ProfScope prof("draw_normal", s, 8.0 * (double)n);
    hipLaunchKernelGGL(normal_kernel, dim3(draw_blocks((long)n)), dim3(DRAW_BS), 0, s, draw_base(seed, epoch, step, kind), first, (long)n, scale, d_out);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

}
