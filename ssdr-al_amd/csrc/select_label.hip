// oracle_labeling (S3/sampler2.py:124-192) over the picks of one round, with the order _help() is called in by sampling() (:676-684, :796-806,
// fps_gcn_cpu.py:172-178), for gfx950: pseudo labels, the click budget, the class list and the counters without a host loop.
//
//   1. order    the items are grouped by cloud, clouds by a key (the caller's, or the first position among the items: atomicMin), picks of a cloud in
//               pick order: a stable radix sort of (key, position).
//   2. verdict  one pass per item over its points: ground-truth histogram in LDS, first maximum like np.argmax, rate = double(count) / double(len)
//               compared with >=.  NAIL below the threshold: the points split by predicted class, every sub-region of MORE than min_size points judged
//               the same way.  Regions of up to 256 points: a WAVE each, four points per lane kept in registers, one 64-entry histogram per wave that
//               is refilled per predicted class present.  Larger regions: a WORKGROUP each, the joint [class][label] histogram (32 x 64) in LDS, one
//               atomic per point.  The verdict is what the item would cost and append, whether or not the budget reaches it.
//   3. scan     exclusive prefix of the costs in item order, one workgroup: item i is processed iff prefix_i < budget.  Costs are >= 0 and the
//               reference never resumes after its break, so this IS the sequential walk, the budget that ends below zero included.  The same pass
//               gives every item its slice of the class list and sums the counters (no atomics: one workgroup).
//   4. apply    processed items write their points, class entries, used flag and labelled-mask byte.  A region picked twice pays twice and writes
//               the same values twice.
// Nothing waits on the host; the scratch is per stream.
// A sharded round runs the same chain in two halves around one all-gather (further down): verdicts of a rank's own items packed into fixed-size
// records, then order / scan / apply over the records of all ranks.
#include "ssdr_internal.hpp"
#include "block_prims.hpp"

namespace ssdr {
namespace {

constexpr int LB_WAVE_MAX = 256;            // largest region of the wave form: 4 points per lane
constexpr size_t LB_MAX_ITEMS = (size_t)1 << 22;
enum { LB_ST_LABEL = 1, LB_ST_CLASS = 2, LB_ST_ITEM = 4, LB_ST_CAP = 8 };

struct LabelArgs {
    const int* gt; const int* pred; long long n; const int* sp_off; const int* sp_pts; const int* sp_cloud; int S, B;
    const int* items; const int* n_items; int max_items;
    int nl, nc, nail; double thr; long long min_size;
    // scratch: per position in processing order
    const unsigned* ord;                       // the item (position among the picks) processed at this position
    int *kind, *lab, *cost, *nent, *subp, *len, *eoff; unsigned* smask; unsigned char* sublab;      // kind: 0 skipped, 1 whole region, 2 split, 3 ignored
    int* big;                                  // positions left to the workgroup form
    int* cnt;                                  // [0] entries of big, [1] status
};

__device__ __forceinline__ int item_count(const LabelArgs& a) { return max(0, min(*a.n_items, a.max_items)); }
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ long long wave_max_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ unsigned wave_or_u(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the cloud of an item, -1 for an id outside the regions / a cloud outside the table
__device__ __forceinline__ int item_cloud(const LabelArgs& a, int sp) {
    if (sp < 0 || sp >= a.S) return -1;
    const int c = a.sp_cloud[sp];
    return c >= 0 && c < a.B ? c : -1;
}

// ---- 1. order ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void label_first(LabelArgs a, int* first) {
    const int M = item_count(a);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < M; i += gridDim.x * 256) {
        const int c = item_cloud(a, a.items[i]);
        if (c < 0) atomicOr(&a.cnt[1], (int)LB_ST_ITEM); else atomicMin(&first[c], i);
    }
}
__global__ __launch_bounds__(256) void label_keys(LabelArgs a, const int* __restrict__ key, unsigned long long* keys, unsigned* vals) {
    const int M = item_count(a);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < M; i += gridDim.x * 256) {
        const int c = item_cloud(a, a.items[i]);
        if (c < 0) atomicOr(&a.cnt[1], (int)LB_ST_ITEM);
        keys[i] = c < 0 ? 0x7fffffffull : (unsigned long long)(unsigned)max(key[c], 0);      // (an item outside the regions does nothing: last)
        vals[i] = (unsigned)i;
    }
}

// ---- 2. verdict --------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_verdict(const LabelArgs& a, int j, int kind, int lab, int cost, int nent, int subp, int len, unsigned smask) {
    a.kind[j] = kind; a.lab[j] = lab; a.cost[j] = cost; a.nent[j] = nent; a.subp[j] = subp; a.len[j] = len; a.smask[j] = smask;
}

__global__ __launch_bounds__(256) void label_verdict_wave(LabelArgs a) {
    __shared__ int s_h[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int M = item_count(a);
    for (int j = blockIdx.x * 4 + w; j < M; j += gridDim.x * 4) {
        const int sp = a.items[a.ord[j]];
        const bool ok = item_cloud(a, sp) >= 0;
        const int lo = ok ? a.sp_off[sp] : 0, n = ok ? a.sp_off[sp + 1] - lo : 0;
        if (n <= 0 || (long long)n < a.min_size) {                      // costs nothing, is not used, does not stop the walk
            if (lane == 0) put_verdict(a, j, 0, 0, 0, 0, 0, max(n, 0), 0u);
            continue;
        }
        if (n > LB_WAVE_MAX) {
            if (lane == 0) a.big[atomicAdd(&a.cnt[0], 1)] = j;
            continue;
        }
        int g[4], c[4], bad = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            g[u] = -1; c[u] = -1;
            const int i = lane + 64 * u;
            if (i < n) {
                const int p = a.sp_pts[lo + i];
                if (p < 0 || p >= a.n) { bad |= LB_ST_ITEM; continue; }
                g[u] = a.gt[p]; c[u] = a.nail ? a.pred[p] : 0;
                if (g[u] < 0 || g[u] >= a.nl) { bad |= LB_ST_LABEL; g[u] = -1; }
                if (c[u] < 0 || c[u] >= a.nc) { bad |= LB_ST_CLASS; c[u] = -1; }
            }
        }
        if (bad) atomicOr(&a.cnt[1], bad);
        s_h[w][lane] = 0;
        wave_sync();
#pragma unroll
        for (int u = 0; u < 4; ++u) if (g[u] >= 0) atomicAdd(&s_h[w][g[u]], 1);
        wave_sync();
        // (count, lowest label first) as one key: the wave's maximum is np.argmax's first maximum
        int key = wave_max_i(lane < a.nl ? (s_h[w][lane] << 6) | (63 - lane) : -1);
        const int lab = 63 - (key & 63);
        int kind = 1, cost = 1, nent = 1, subp = 0; unsigned smask = 0u;
        if (a.nail && !((double)(key >> 6) / (double)n >= a.thr)) {
            unsigned m = 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) if (c[u] >= 0) m |= 1u << c[u];
            m = wave_or_u(m);
            while (m) {                                                 // the predicted classes present, ascending
                const int k = __ffsll((unsigned long long)m) - 1;
                m &= m - 1u;
                s_h[w][lane] = 0;
                wave_sync();
                int mine = 0;
#pragma unroll
                for (int u = 0; u < 4; ++u) if (c[u] == k) { ++mine; if (g[u] >= 0) atomicAdd(&s_h[w][g[u]], 1); }
                wave_sync();
                const int sub = wave_sum(mine);
                key = wave_max_i(lane < a.nl ? (s_h[w][lane] << 6) | (63 - lane) : -1);
                if ((long long)sub > a.min_size && (double)(key >> 6) / (double)sub >= a.thr) {      // strictly more than min_size
                    smask |= 1u << k; subp += sub;
                    if (lane == 0) a.sublab[(size_t)j * 32 + k] = (unsigned char)(63 - (key & 63));
                }
            }
            nent = __popc(smask); cost = 1 + nent; kind = smask ? 2 : 3;
        }
        if (lane == 0) put_verdict(a, j, kind, lab, cost, nent, subp, n, smask);
    }
}

__global__ __launch_bounds__(256) void label_verdict_block(LabelArgs a) {
    __shared__ int s_j[32][64];             // [predicted class][label]; dominant mode: row 0 alone
    __shared__ int s_nolab[32];             // points of a class whose label is out of range: they count for the sub-region's length
    __shared__ int s_sl[32];
    __shared__ long long s_top;
    __shared__ unsigned s_mask;
    __shared__ int s_subp;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nb = a.cnt[0], rows = a.nail ? a.nc : 1;
    for (int b = blockIdx.x; b < nb; b += gridDim.x) {
        const int j = a.big[b], sp = a.items[a.ord[j]];
        const int lo = a.sp_off[sp], n = a.sp_off[sp + 1] - lo;
        for (int i = tid; i < 32 * 64; i += 256) (&s_j[0][0])[i] = 0;
        if (tid < 32) s_nolab[tid] = 0;
        if (tid == 0) { s_mask = 0u; s_subp = 0; }
        __syncthreads();
        int bad = 0;
        for (int i = tid; i < n; i += 256) {
            const int p = a.sp_pts[lo + i];
            if (p < 0 || p >= a.n) { bad |= LB_ST_ITEM; continue; }
            const int g = a.gt[p], c = a.nail ? a.pred[p] : 0;
            const bool gok = g >= 0 && g < a.nl, cok = c >= 0 && c < a.nc;
            if (!gok) bad |= LB_ST_LABEL;
            if (!cok) bad |= LB_ST_CLASS;
            if (cok) atomicAdd(gok ? &s_j[c][g] : &s_nolab[c], 1);
        }
        if (bad) atomicOr(&a.cnt[1], bad);
        __syncthreads();
        if (w == 0) {
            long long cnt = 0;
            for (int c = 0; c < rows; ++c) cnt += s_j[c][lane];
            const long long key = wave_max_ll(lane < a.nl ? (cnt << 6) | (long long)(63 - lane) : -1ll);
            if (lane == 0) s_top = key;
        }
        __syncthreads();
        const long long top = s_top;
        const bool pass = !a.nail || (double)(top >> 6) / (double)n >= a.thr;
        if (!pass) {
            for (int k = w; k < a.nc; k += 4) {
                const int v = s_j[k][lane];
                const int sub = wave_sum(v) + s_nolab[k];
                const int key = wave_max_i(lane < a.nl ? (v << 6) | (63 - lane) : -1);        // (a region below 2^25 points: the count fits above the label)
                if (lane == 0 && sub > 0 && (long long)sub > a.min_size && (double)(key >> 6) / (double)sub >= a.thr) {
                    atomicOr(&s_mask, 1u << k); atomicAdd(&s_subp, sub); s_sl[k] = 63 - (key & 63);
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const unsigned sm = pass ? 0u : s_mask;
            const int nent = pass ? 1 : __popc(sm);
            put_verdict(a, j, pass ? 1 : (sm ? 2 : 3), (int)(63 - (top & 63)), pass ? 1 : 1 + nent, nent, pass ? 0 : s_subp, n, sm);
        }
        if (!pass && tid < 32 && ((s_mask >> tid) & 1u)) a.sublab[(size_t)j * 32 + tid] = (unsigned char)s_sl[tid];
        __syncthreads();                    // the histograms are cleared for the next region
    }
}

// ---- 3. scan -----------------------------------------------------------------------------------------------------------------------------------
// out[0..5] sp_num, p_num, sub_num, sub_p_num, split_sp_num, ignore_sp_num; [6] class entries appended; [7] budget left; [8] status; [9] items used;
// [10], [11] regions judged by the wave / the workgroup form (all items, processed or not)
__global__ __launch_bounds__(1024) void label_scan(LabelArgs a, long long* budget_io, long long class_cap, long long* out) {
    __shared__ long long s_c[16], s_e[16], s_r[16][8];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int M = item_count(a);
    const long long budget = *budget_io;
    if (tid == 0) { out[6] = 0; out[7] = budget; }
    long long runc = 0, rune = 0, ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int base = 0; base < M; base += 1024) {
        const int j = base + tid;
        const long long cost = j < M ? a.cost[j] : 0, ne = j < M ? a.nent[j] : 0;
        long long ic = cost, ie = ne;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long tc = __shfl_up(ic, (unsigned)o), te = __shfl_up(ie, (unsigned)o);
            if (lane >= o) { ic += tc; ie += te; }
        }
        if (lane == 63) { s_c[w] = ic; s_e[w] = ie; }
        __syncthreads();                    // (also orders thread 0's defaults before the last processed item's totals)
        long long pc = 0, pe = 0, tc = 0, te = 0;
        for (int q = 0; q < 16; ++q) { if (q < w) { pc += s_c[q]; pe += s_e[q]; } tc += s_c[q]; te += s_e[q]; }
        const long long exc = runc + pc + ic - cost, exe = rune + pe + ie - ne;
        if (j < M) {
            const bool proc = exc < budget;                             // budget["click"] > 0 when the walk reaches the item
            const int kind = a.kind[j];
            a.eoff[j] = proc ? (int)min(exe, (long long)0x7fffffff) : -1;
            if (kind) ctr[a.len[j] > LB_WAVE_MAX ? 7 : 6] += 1;
            if (proc) {
                if (kind == 1) { ctr[0] += 1; ctr[1] += a.len[j]; }
                if (kind == 2) { ctr[2] += ne; ctr[3] += a.subp[j]; ctr[4] += 1; }
                if (kind == 3) ctr[5] += 1;
                if (j == M - 1 || exc + cost >= budget) {               // the last item the walk processes: the totals
                    out[6] = exe + ne; out[7] = budget - (exc + cost); *budget_io = budget - (exc + cost);
                    if (exe + ne > class_cap) atomicOr(&a.cnt[1], (int)LB_ST_CAP);
                }
            }
        }
        runc += tc; rune += te;
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) { const long long v = wave_sum_ll(ctr[q]); if (lane == 0) s_r[w][q] = v; }
    __syncthreads();
    if (tid == 0) {
        long long t[8];
        for (int c = 0; c < 8; ++c) { t[c] = 0; for (int q = 0; q < 16; ++q) t[c] += s_r[q][c]; }
        for (int c = 0; c < 6; ++c) out[c] = t[c];
        out[8] = a.cnt[1]; out[9] = t[0] + t[4] + t[5]; out[10] = t[6]; out[11] = t[7];
    }
}

// ---- 4. apply ----------------------------------------------------------------------------------------------------------------------------------
struct LabelOut { float* mask; float* label; unsigned char* used; unsigned char* labeled; int* class_out; long long class_cap; int* proc_order; };

// (the record path's: apply_item of the one-call chain keeps its own loops)
// thread t of nt writes the points [lo, lo + n) of a region judged `kind` (1: whole, 2: split by predicted class with the sub-regions' labels sl)
__device__ __forceinline__ void apply_points(const int* __restrict__ sp_pts, const int* __restrict__ pred, long long npts, int nc, const LabelOut& o, int kind, int lab,
                                             unsigned sm, const unsigned char* sl, int lo, int n, int t, int nt) {
    if (kind == 1) {
        const float v = (float)lab;
        for (int i = t; i < n; i += nt) { const int p = sp_pts[lo + i]; if (p >= 0 && p < npts) { o.mask[p] = 1.0f; o.label[p] = v; } }
    } else if (kind == 2) {
        for (int i = t; i < n; i += nt) {
            const int p = sp_pts[lo + i];
            if (p < 0 || p >= npts) continue;
            const int c = pred[p];
            if (c >= 0 && c < nc && ((sm >> c) & 1u)) { o.mask[p] = 1.0f; o.label[p] = (float)sl[c]; }
        }
    }
}
// thread t of nt working on position j
__device__ __forceinline__ void apply_item(const LabelArgs& a, const LabelOut& o, int j, int t, int nt) {
    const int e = a.eoff[j], kind = a.kind[j];
    if (e < 0 || kind == 0) return;
    const int oi = (int)a.ord[j], sp = a.items[oi];
    const int lo = a.sp_off[sp], n = a.sp_off[sp + 1] - lo;
    const unsigned sm = a.smask[j];
    const unsigned char* sl = a.sublab + (size_t)j * 32;
    if (t == 0) {
        o.used[oi] = 1; o.labeled[sp] = 1;
        if ((long long)e + a.nent[j] <= o.class_cap) {
            if (kind == 1) o.class_out[e] = a.lab[j];
            if (kind == 2) { int r = 0; for (int k = 0; k < 32; ++k) if ((sm >> k) & 1u) o.class_out[e + r++] = sl[k]; }      // ascending class: the reference's order
        }
    }
    if (kind == 1) {
        const float v = (float)a.lab[j];
        for (int i = t; i < n; i += nt) { const int p = a.sp_pts[lo + i]; if (p >= 0 && p < a.n) { o.mask[p] = 1.0f; o.label[p] = v; } }
    } else if (kind == 2) {
        for (int i = t; i < n; i += nt) {
            const int p = a.sp_pts[lo + i];
            if (p < 0 || p >= a.n) continue;
            const int c = a.pred[p];
            if (c >= 0 && c < a.nc && ((sm >> c) & 1u)) { o.mask[p] = 1.0f; o.label[p] = (float)sl[c]; }
        }
    }
}
__global__ __launch_bounds__(256) void label_apply_wave(LabelArgs a, LabelOut o) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int M = item_count(a);
    for (int j = blockIdx.x * 4 + w; j < M; j += gridDim.x * 4) {
        if (lane == 0 && o.proc_order) o.proc_order[j] = (int)a.ord[j];
        if (a.len[j] <= LB_WAVE_MAX) apply_item(a, o, j, lane, 64);
    }
}
__global__ __launch_bounds__(256) void label_apply_block(LabelArgs a, LabelOut o) {
    const int nb = a.cnt[0];
    for (int b = blockIdx.x; b < nb; b += gridDim.x) apply_item(a, o, a.big[b], threadIdx.x, 256);
}

// ---- the chain in two halves: a sharded round ----------------------------------------------------------------------------------------------------
// A rank judges its own items (verdict half) and packs one fixed-size record per item slot; the records of all ranks are gathered; every rank sorts
// them by their walk key, runs the scan above over ALL of them (costs depend on the item alone, so the replicated prefix sum is the sequential walk)
// and applies its own (walk half).  Dead slots (beyond a rank's live count) carry an all-ones key and cost nothing: they sort last.
struct LabelRecord {
    unsigned long long key;                    // 0: cloud key << 32 | position in pick order
    int pos, kind, lab, cost, nent, subp, len; // 8: the slot among the rank's items; 12 .. 35: the verdict
    unsigned smask;                            // 36: the sub-regions (predicted classes) that are labelled
    unsigned char sublab[32];                  // 40: their labels (0 where the mask is clear)
    int status, pad;                           // 72: the status bits the rank's verdict half raised
};
static_assert(sizeof(LabelRecord) == SSDR_LABEL_RECORD_BYTES && SSDR_LABEL_RECORD_BYTES % 16 == 0, "record layout (ssdr_al.h)");
constexpr unsigned long long LB_DEAD_KEY = ~0ull;

__global__ __launch_bounds__(256) void label_ident(LabelArgs a, unsigned* ord) {
    const int M = item_count(a);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.max_items; i += gridDim.x * 256) {
        ord[i] = (unsigned)i;
        if (i < M && item_cloud(a, a.items[i]) < 0) atomicOr(&a.cnt[1], (int)LB_ST_ITEM);
    }
}
__global__ __launch_bounds__(256) void label_pack(LabelArgs a, const unsigned long long* __restrict__ keys, LabelRecord* rec) {
    const int M = item_count(a), st = a.cnt[1];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.max_items; i += gridDim.x * 256) {
        LabelRecord r;
        const bool live = i < M;
        const int kind = live ? a.kind[i] : 0;
        r.key = live ? keys[i] : LB_DEAD_KEY; r.pos = i; r.kind = kind;
        r.lab = live ? a.lab[i] : 0; r.cost = live ? a.cost[i] : 0; r.nent = live ? a.nent[i] : 0; r.subp = live ? a.subp[i] : 0; r.len = live ? a.len[i] : 0;
        r.smask = kind == 2 ? a.smask[i] : 0u;
#pragma unroll
        for (int k = 0; k < 32; ++k) r.sublab[k] = (r.smask >> k) & 1u ? a.sublab[(size_t)i * 32 + k] : (unsigned char)0;
        r.status = st; r.pad = 0;
        rec[i] = r;
    }
}

struct WalkArgs {
    const LabelRecord* rec; int total, max_items, rank;                  // all ranks' records, rank-major
    const unsigned* ord;                                                   // the record at every position of the walk
    const int* pred; long long n; const int* sp_off; const int* sp_pts; int S, nc;
    const int* items; const int* n_items;                                // this rank's
    int* eoff; int* big; int* cnt; int* walk_pos;
};
__global__ __launch_bounds__(256) void label_record_keys(WalkArgs a, unsigned long long* keys, unsigned* vals) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.total; i += gridDim.x * 256) {
        keys[i] = a.rec[i].key; vals[i] = (unsigned)i;
        if (i % a.max_items == 0 && a.rec[i].status) atomicOr(&a.cnt[1], a.rec[i].status & (LB_ST_LABEL | LB_ST_CLASS | LB_ST_ITEM));      // a rank's bits ride in its records
    }
}
// label_scan over all ranks' records through their sorted order (dead records: no cost, no entry, kind 0)
__global__ __launch_bounds__(1024) void label_scan_records(WalkArgs a, long long* budget_io, long long class_cap, long long* out) {
    __shared__ long long s_c[16], s_e[16], s_r[16][8];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int M = a.total;
    const long long budget = *budget_io;
    if (tid == 0) { out[6] = 0; out[7] = budget; }
    long long runc = 0, rune = 0, ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int base = 0; base < M; base += 1024) {
        const int j = base + tid;
        const long long cost = j < M ? max(a.rec[a.ord[j]].cost, 0) : 0, ne = j < M ? max(a.rec[a.ord[j]].nent, 0) : 0;
        long long ic = cost, ie = ne;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long tc = __shfl_up(ic, (unsigned)o), te = __shfl_up(ie, (unsigned)o);
            if (lane >= o) { ic += tc; ie += te; }
        }
        if (lane == 63) { s_c[w] = ic; s_e[w] = ie; }
        __syncthreads();                    // (also orders thread 0's defaults before the last processed item's totals)
        long long pc = 0, pe = 0, tc = 0, te = 0;
        for (int q = 0; q < 16; ++q) { if (q < w) { pc += s_c[q]; pe += s_e[q]; } tc += s_c[q]; te += s_e[q]; }
        const long long exc = runc + pc + ic - cost, exe = rune + pe + ie - ne;
        if (j < M) {
            const bool proc = exc < budget;                             // budget["click"] > 0 when the walk reaches the item
            const LabelRecord& q = a.rec[a.ord[j]];
            const int kind = q.kind;
            a.eoff[j] = proc ? (int)min(exe, (long long)0x7fffffff) : -1;
            if (kind) ctr[q.len > LB_WAVE_MAX ? 7 : 6] += 1;
            if (proc) {
                if (kind == 1) { ctr[0] += 1; ctr[1] += q.len; }
                if (kind == 2) { ctr[2] += ne; ctr[3] += q.subp; ctr[4] += 1; }
                if (kind == 3) ctr[5] += 1;
                if (j == M - 1 || exc + cost >= budget) {               // the last item the walk processes: the totals
                    out[6] = exe + ne; out[7] = budget - (exc + cost); *budget_io = budget - (exc + cost);
                    if (exe + ne > class_cap) atomicOr(&a.cnt[1], (int)LB_ST_CAP);
                }
            }
        }
        runc += tc; rune += te;
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) { const long long v = wave_sum_ll(ctr[q]); if (lane == 0) s_r[w][q] = v; }
    __syncthreads();
    if (tid == 0) {
        long long t[8];
        for (int c = 0; c < 8; ++c) { t[c] = 0; for (int q = 0; q < 16; ++q) t[c] += s_r[q][c]; }
        for (int c = 0; c < 6; ++c) out[c] = t[c];
        out[8] = a.cnt[1]; out[9] = t[0] + t[4] + t[5]; out[10] = t[6]; out[11] = t[7];
    }
}
// the class list from ALL records (identical on every rank); this rank's own records: walk position, used flag, labelled byte, points
__device__ __forceinline__ bool walk_own(const WalkArgs& a, unsigned r, int& slot, int& sp, int& lo, int& n) {
    slot = (int)(r % (unsigned)a.max_items);
    if ((int)(r / (unsigned)a.max_items) != a.rank || slot >= max(0, min(*a.n_items, a.max_items))) return false;
    sp = a.items[slot];
    if (sp < 0 || sp >= a.S) return false;
    lo = a.sp_off[sp]; n = a.sp_off[sp + 1] - lo;
    return true;
}
__global__ __launch_bounds__(256) void label_walk_apply_wave(WalkArgs a, LabelOut o) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int j = blockIdx.x * 4 + w; j < a.total; j += gridDim.x * 4) {
        const unsigned r = a.ord[j];
        const LabelRecord& q = a.rec[r];
        const int e = a.eoff[j];
        if (e < 0 || q.key == LB_DEAD_KEY) continue;
        int slot, sp, lo, n;
        const bool own = walk_own(a, r, slot, sp, lo, n);
        if (lane == 0) {
            if (own) a.walk_pos[slot] = j;
            if ((long long)e + max(q.nent, 0) <= o.class_cap) {           // (all of an item's entries or none, as the one-call chain)
                if (q.kind == 1 && e < o.class_cap) o.class_out[e] = q.lab;
                if (q.kind == 2) { int c = 0; for (int k = 0; k < 32; ++k) if ((q.smask >> k) & 1u) { if ((long long)e + c < o.class_cap) o.class_out[e + c] = q.sublab[k]; ++c; } }
            }
        }
        if (!own || (q.kind != 1 && q.kind != 2 && q.kind != 3)) continue;
        if (lane == 0) { o.used[slot] = 1; o.labeled[sp] = 1; }
        if (q.kind == 3 || (q.kind == 2 && !a.pred)) continue;
        if (n > LB_WAVE_MAX) { if (lane == 0) a.big[atomicAdd(&a.cnt[0], 1)] = j; continue; }
        apply_points(a.sp_pts, a.pred, a.n, a.nc, o, q.kind, q.lab, q.smask, q.sublab, lo, n, lane, 64);
    }
}
__global__ __launch_bounds__(256) void label_walk_apply_block(WalkArgs a, LabelOut o) {
    const int nb = min(a.cnt[0], a.max_items);
    for (int b = blockIdx.x; b < nb; b += gridDim.x) {
        const unsigned r = a.ord[a.big[b]];
        const LabelRecord& q = a.rec[r];
        int slot, sp, lo, n;
        if (walk_own(a, r, slot, sp, lo, n)) apply_points(a.sp_pts, a.pred, a.n, a.nc, o, q.kind, q.lab, q.smask, q.sublab, lo, n, threadIdx.x, 256);
    }
}

// ---- walk keys of a sharded round: cloud key << 32 | position in pick order ----------------------------------------------------------------------------
// fps / k-center: the picks (indices into the global candidate list, both replicated); a cloud's key is its first appearance among ALL picks
__global__ __launch_bounds__(256) void label_pick_first(const int* __restrict__ picks, int n_picks, const int* __restrict__ n_cand, const int* __restrict__ cand, int cand_cap,
                                                        const int* __restrict__ gcloud, long long G, int NB, int* first) {
    const int ng = max(0, min(*n_cand, cand_cap));
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_picks; i += gridDim.x * 256) {
        const int s = picks[i];
        if (s < 0 || s >= ng) continue;
        const int g = cand[s];
        if (g < 0 || g >= G) continue;
        const int c = gcloud[g];
        if (c >= 0 && c < NB) atomicMin(&first[c], i);
    }
}
// ... and this rank's share of them, in pick order: an ordered compaction by one workgroup
__global__ __launch_bounds__(1024) void label_own_picks(const int* __restrict__ picks, int n_picks, const int* __restrict__ n_cand, const int* __restrict__ cand, int cand_cap,
                                                        const int* __restrict__ gcloud, long long G, int NB, const int* __restrict__ first, int rank, int Smax,
                                                        int max_items, int* items, int* n_items, unsigned long long* keys) {
    __shared__ int s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ng = max(0, min(*n_cand, cand_cap));
    int run = 0;
    for (int base = 0; base < n_picks; base += 1024) {
        const int i = base + tid;
        int g = -1;
        if (i < n_picks) { const int s = picks[i]; if (s >= 0 && s < ng) g = cand[s]; }
        const bool mine = g >= 0 && g < G && g / Smax == rank;
        const unsigned long long b = __ballot(mine);
        if (lane == 0) s_w[w] = __popcll(b);
        __syncthreads();
        int before = run, tot = 0;
        for (int q = 0; q < 16; ++q) { if (q < w) before += s_w[q]; tot += s_w[q]; }
        const int at = before + __popcll(b & ((1ull << lane) - 1ull));
        if (mine && at < max_items) {
            const int c = gcloud[g];
            const unsigned long long hi = c >= 0 && c < NB ? (unsigned long long)(unsigned)max(first[c], 0) : 0x7fffffffull;
            items[at] = g - rank * Smax; keys[at] = (hi << 32) | (unsigned long long)(unsigned)i;
        }
        run += tot;
        __syncthreads();
    }
    if (tid == 0) *n_items = min(run, max_items);
}
// edcd / topk: a rank holds its own picks; the cloud key is the caller's (per global cloud), the low half the position among the rank's picks
__global__ __launch_bounds__(256) void label_item_keys(const int* __restrict__ items, const int* __restrict__ n_items, int max_items, const int* __restrict__ gcloud, int rank,
                                                       int Smax, int NB, const int* __restrict__ cloud_key, unsigned long long* keys) {
    const int M = max(0, min(*n_items, max_items));
    for (int i = blockIdx.x * 256 + threadIdx.x; i < M; i += gridDim.x * 256) {
        const int sp = items[i];
        const int c = sp >= 0 && sp < Smax ? gcloud[(long long)rank * Smax + sp] : -1;
        const unsigned long long hi = c >= 0 && c < NB ? (unsigned long long)(unsigned)max(cloud_key[c], 0) : 0x7fffffffull;
        keys[i] = (hi << 32) | (unsigned long long)(unsigned)i;
    }
}

// ---- the picks of a one-call selection chain as items --------------------------------------------------------------------------------------------
// layout 0: d_result of ssdr_gcn_fps_sampling_dev / ssdr_edcd_sampling_dev (counts, picks at word 8 as indices into the candidate list behind them);
// layout 1: ssdr_topk_regions_dev's (count in word 0, region ids from word 8)
__global__ __launch_bounds__(256) void label_items(const int* __restrict__ res, int layout, int max_select, int max_items, int* items, int* n_items) {
    const int count = max(0, min(layout == 0 ? (res[5] ? 0 : res[4]) : res[0], min(max_items, max_select)));
    const int n_unl = res[0];
    const int* cand = res + 8 + max_select;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const int s = res[8 + i];
        items[i] = layout == 0 ? (s >= 0 && s < n_unl ? cand[s] : -1) : s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_items = count;
}
// a cloud's key for the edcd round: its first place in the ranking among the regions that compete (file_list_top's order, sampler2.py:533-552)
__global__ __launch_bounds__(256) void label_rank_key(const int* __restrict__ order, int S, const unsigned char* __restrict__ skip, const int* __restrict__ sp_cloud, int B, int* key) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < S; r += gridDim.x * 256) {
        const int id = order[r];
        if (id < 0 || id >= S || (skip && skip[id])) continue;
        const int c = sp_cloud[id];
        if (c >= 0 && c < B) atomicMin(&key[c], r);
    }
}

struct LabelState { RadixSorter sorter; DevBuf keys, vals, first, verdict, sublab, big, cnt; };
LabelState& lst(hipStream_t s) { return per_stream<LabelState>(s); }
unsigned grid_of(size_t work, size_t per_block, int waves) { return (unsigned)std::max<size_t>(1, std::min<size_t>((work + per_block - 1) / per_block, (size_t)ctx().num_cu * waves)); }

}  // namespace
}  // namespace ssdr

using namespace ssdr;

extern "C" {

int ssdr_oracle_label_dev(const int32_t* d_gt, const int32_t* d_pred_class, size_t n, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t S,
                          const int32_t* d_sp_cloud, size_t num_clouds, const int32_t* d_items, const int32_t* d_n_items, size_t max_items,
                          const int32_t* d_cloud_key, size_t max_region, int num_labels, int num_classes, int mode, double threshold, int64_t min_size,
                          int64_t* d_budget, float* d_mask, float* d_label, uint8_t* d_used, uint8_t* d_labeled, int32_t* d_class_out, size_t class_cap,
                          int32_t* d_proc_order, int64_t* d_out, void* stream) {
    if (mode != SSDR_LABEL_DOMINANT && mode != SSDR_LABEL_NAIL) { set_error("oracle_label: unknown oracle mode %d (0: dominant, 1: NAIL)", mode); return SSDR_ERR_INVALID; }
    if (!d_gt || !d_sp_off || !d_sp_pts || !d_sp_cloud || !d_n_items || !d_budget || !d_mask || !d_label || !d_used || !d_labeled || !d_class_out || !d_out ||
        (max_items && !d_items) || (mode == SSDR_LABEL_NAIL && !d_pred_class) || num_labels < 1 || num_labels > 64 || num_classes < 1 || num_classes > 32 ||
        max_items > LB_MAX_ITEMS || S > 0x7ffffff0 || num_clouds > 0x7ffffff0 || n > 0x7ffffff0 || !(threshold == threshold)) {
        set_error("oracle_label: bad arguments (num_labels <= 64, num_classes <= 32, at most 2^22 items)"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); LabelState& Q = lst(s);
    const size_t M = max_items, Mp = std::max<size_t>(M, 1);
    SSDR_TRY(Q.keys.reserve(8 * Mp)); SSDR_TRY(Q.vals.reserve(4 * Mp)); SSDR_TRY(Q.first.reserve(4 * std::max<size_t>(num_clouds, 1)));
    SSDR_TRY(Q.verdict.reserve(4 * 8 * Mp)); SSDR_TRY(Q.sublab.reserve(32 * Mp)); SSDR_TRY(Q.big.reserve(4 * Mp)); SSDR_TRY(Q.cnt.reserve(64));
    int* v = Q.verdict.as<int>();
    LabelArgs a{d_gt, d_pred_class, (long long)n, d_sp_off, d_sp_pts, d_sp_cloud, (int)S, (int)num_clouds, d_items, d_n_items, (int)M,
                num_labels, num_classes, mode == SSDR_LABEL_NAIL ? 1 : 0, threshold, (long long)min_size,
                Q.vals.as<unsigned>(), v, v + Mp, v + 2 * Mp, v + 3 * Mp, v + 4 * Mp, v + 5 * Mp, v + 6 * Mp, reinterpret_cast<unsigned*>(v + 7 * Mp),
                Q.sublab.as<unsigned char>(), Q.big.as<int>(), Q.cnt.as<int>()};
    LabelOut o{d_mask, d_label, d_used, d_labeled, d_class_out, (long long)std::min<size_t>(class_cap, (size_t)1 << 40), d_proc_order};
    SSDR_HIP(hipMemsetAsync(Q.cnt.p, 0, 64, s));
    if (M) {
        SSDR_HIP(hipMemsetAsync(d_used, 0, M, s));
        {
            ProfScope prof("label_order", s, 16.0 * (double)M);
            const unsigned g = grid_of(M, 256, 16);
            const int* key = d_cloud_key;
            int bits = 31;
            if (!key) {                       // first appearance among the items
                SSDR_HIP(hipMemsetAsync(Q.first.p, 0x7f, 4 * std::max<size_t>(num_clouds, 1), s));
                hipLaunchKernelGGL(label_first, dim3(g), dim3(256), 0, s, a, Q.first.as<int>());
                key = Q.first.as<int>();
            }
            hipLaunchKernelGGL(label_keys, dim3(g), dim3(256), 0, s, a, key, Q.keys.as<unsigned long long>(), Q.vals.as<unsigned>());
            SSDR_TRY(Q.sorter.sort(Q.keys.as<uint64_t>(), Q.vals.as<uint32_t>(), (int)M, d_n_items, s, bits));
        }
        const bool blocks = max_region == 0 || max_region > (size_t)LB_WAVE_MAX;      // max_region: the caller's bound on a region's size (0: none)
        {
            ProfScope prof("label_form:wave", s, 0.0);
            hipLaunchKernelGGL(label_verdict_wave, dim3(grid_of(M, 4, 16)), dim3(256), 0, s, a);
        }
        if (blocks) {
            ProfScope prof("label_form:block", s, 0.0);
            hipLaunchKernelGGL(label_verdict_block, dim3(grid_of(M, 1, 4)), dim3(256), 0, s, a);
        }
    }
    {
        ProfScope prof("label_scan", s, 0.0);
        hipLaunchKernelGGL(label_scan, dim3(1), dim3(1024), 0, s, a, (long long*)d_budget, o.class_cap, (long long*)d_out);
    }
    if (M) {
        ProfScope prof("label_apply", s, 0.0);
        hipLaunchKernelGGL(label_apply_wave, dim3(grid_of(M, 4, 16)), dim3(256), 0, s, a, o);
        if (max_region == 0 || max_region > (size_t)LB_WAVE_MAX) hipLaunchKernelGGL(label_apply_block, dim3(grid_of(M, 1, 4)), dim3(256), 0, s, a, o);
    }
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_oracle_label_items_dev(const int32_t* d_result, int layout, size_t max_select, const int32_t* d_order, size_t S, const uint8_t* d_skip,
                                const int32_t* d_sp_cloud, size_t num_clouds, int32_t* d_items, size_t max_items, int32_t* d_n_items, int32_t* d_cloud_key,
                                void* stream) {
    if ((d_result && (layout < 0 || layout > 1 || !d_items || !d_n_items)) || max_items > LB_MAX_ITEMS || max_select > 0x7ffffff0 || S > 0x7ffffff0 ||
        num_clouds > 0x7ffffff0 || (d_cloud_key && (!d_order || !d_sp_cloud)) || (!d_result && !d_cloud_key)) {
        set_error("oracle_label_items: bad arguments"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    ProfScope prof("label_items", s, 0.0);
    if (d_result) hipLaunchKernelGGL(label_items, dim3(grid_of(std::max<size_t>(max_items, 1), 256, 16)), dim3(256), 0, s, d_result, layout, (int)max_select, (int)max_items, d_items, d_n_items);
    if (d_cloud_key && num_clouds) {
        SSDR_HIP(hipMemsetAsync(d_cloud_key, 0x7f, 4 * num_clouds, s));
        if (S) hipLaunchKernelGGL(label_rank_key, dim3(grid_of(S, 256, 16)), dim3(256), 0, s, d_order, (int)S, d_skip, d_sp_cloud, (int)num_clouds, d_cloud_key);
    }
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_oracle_label_verdict_dev(const int32_t* d_gt, const int32_t* d_pred_class, size_t n, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t S,
                                  const int32_t* d_items, const int32_t* d_n_items, size_t max_items, const uint64_t* d_keys, size_t max_region, int num_labels,
                                  int num_classes, int mode, double threshold, int64_t min_size, void* d_records, void* stream) {
    if (mode != SSDR_LABEL_DOMINANT && mode != SSDR_LABEL_NAIL) { set_error("oracle_label_verdict: unknown oracle mode %d (0: dominant, 1: NAIL)", mode); return SSDR_ERR_INVALID; }
    if (!d_gt || !d_sp_off || !d_sp_pts || !d_n_items || (max_items && (!d_items || !d_keys || !d_records)) || (mode == SSDR_LABEL_NAIL && !d_pred_class) || num_labels < 1 ||
        num_labels > 64 || num_classes < 1 || num_classes > 32 || max_items > LB_MAX_ITEMS || S > 0x7ffffff0 || n > 0x7ffffff0 || !(threshold == threshold)) {
        set_error("oracle_label_verdict: bad arguments (num_labels <= 64, num_classes <= 32, at most 2^22 items)"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); LabelState& Q = lst(s);
    const size_t M = max_items, Mp = std::max<size_t>(M, 1);
    if (!M) return SSDR_OK;
    SSDR_TRY(Q.vals.reserve(4 * Mp)); SSDR_TRY(Q.verdict.reserve(4 * 8 * Mp)); SSDR_TRY(Q.sublab.reserve(32 * Mp)); SSDR_TRY(Q.big.reserve(4 * Mp)); SSDR_TRY(Q.cnt.reserve(64));
    SSDR_TRY(Q.first.reserve(4 * std::max<size_t>(S, 1)));      // the verdict kernels ask for an item's cloud: here every region is cloud 0 of one
    SSDR_HIP(hipMemsetAsync(Q.first.p, 0, 4 * std::max<size_t>(S, 1), s));
    int* v = Q.verdict.as<int>();
    LabelArgs a{d_gt, d_pred_class, (long long)n, d_sp_off, d_sp_pts, Q.first.as<int>(), (int)S, 1, d_items, d_n_items, (int)M,
                num_labels, num_classes, mode == SSDR_LABEL_NAIL ? 1 : 0, threshold, (long long)min_size,
                Q.vals.as<unsigned>(), v, v + Mp, v + 2 * Mp, v + 3 * Mp, v + 4 * Mp, v + 5 * Mp, v + 6 * Mp, reinterpret_cast<unsigned*>(v + 7 * Mp),
                Q.sublab.as<unsigned char>(), Q.big.as<int>(), Q.cnt.as<int>()};
    SSDR_HIP(hipMemsetAsync(Q.cnt.p, 0, 64, s));
    hipLaunchKernelGGL(label_ident, dim3(grid_of(M, 256, 16)), dim3(256), 0, s, a, Q.vals.as<unsigned>());
    {
        ProfScope prof("label_form:wave", s, 0.0);
        hipLaunchKernelGGL(label_verdict_wave, dim3(grid_of(M, 4, 16)), dim3(256), 0, s, a);
    }
    if (max_region == 0 || max_region > (size_t)LB_WAVE_MAX) {
        ProfScope prof("label_form:block", s, 0.0);
        hipLaunchKernelGGL(label_verdict_block, dim3(grid_of(M, 1, 4)), dim3(256), 0, s, a);
    }
    {
        ProfScope prof("label_pack", s, (double)SSDR_LABEL_RECORD_BYTES * (double)M);
        hipLaunchKernelGGL(label_pack, dim3(grid_of(M, 256, 16)), dim3(256), 0, s, a, (const unsigned long long*)d_keys, reinterpret_cast<LabelRecord*>(d_records));
    }
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_oracle_label_walk_dev(const void* d_records, int rank, int world, const int32_t* d_pred_class, size_t n, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t S,
                               const int32_t* d_items, const int32_t* d_n_items, size_t max_items, size_t max_region, int num_classes, int64_t* d_budget, float* d_mask,
                               float* d_label, uint8_t* d_used, uint8_t* d_labeled, int32_t* d_class_out, size_t class_cap, int32_t* d_walk_pos, int64_t* d_out,
                               void* stream) {
    if (world < 1 || world > 4096 || rank < 0 || rank >= world || !d_sp_off || !d_sp_pts || !d_n_items || !d_budget || !d_mask || !d_label || !d_used || !d_labeled ||
        !d_class_out || !d_out || !d_walk_pos || (max_items && (!d_items || !d_records)) || num_classes < 1 || num_classes > 32 || max_items > LB_MAX_ITEMS ||
        (size_t)world * max_items > ((size_t)1 << 26) || S > 0x7ffffff0 || n > 0x7ffffff0) {
        set_error("oracle_label_walk: bad arguments (0 <= rank < world, num_classes <= 32, at most 2^22 items per rank and 2^26 records)"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); LabelState& Q = lst(s);
    const size_t M = max_items, T = (size_t)world * M, Tp = std::max<size_t>(T, 1);
    SSDR_TRY(Q.keys.reserve(8 * Tp)); SSDR_TRY(Q.vals.reserve(4 * Tp)); SSDR_TRY(Q.verdict.reserve(4 * Tp)); SSDR_TRY(Q.big.reserve(4 * std::max<size_t>(M, 1))); SSDR_TRY(Q.cnt.reserve(64));
    WalkArgs a{reinterpret_cast<const LabelRecord*>(d_records), (int)T, (int)M, rank, Q.vals.as<unsigned>(), d_pred_class, (long long)n, d_sp_off, d_sp_pts, (int)S, num_classes,
               d_items, d_n_items, Q.verdict.as<int>(), Q.big.as<int>(), Q.cnt.as<int>(), d_walk_pos};
    LabelOut o{d_mask, d_label, d_used, d_labeled, d_class_out, (long long)std::min<size_t>(class_cap, (size_t)1 << 40), nullptr};
    SSDR_HIP(hipMemsetAsync(Q.cnt.p, 0, 64, s));
    if (T) {
        SSDR_HIP(hipMemsetAsync(d_used, 0, M, s));
        SSDR_HIP(hipMemsetAsync(d_walk_pos, 0xff, 4 * M, s));
        ProfScope prof("label_order", s, 16.0 * (double)T);
        hipLaunchKernelGGL(label_record_keys, dim3(grid_of(T, 256, 16)), dim3(256), 0, s, a, Q.keys.as<unsigned long long>(), Q.vals.as<unsigned>());
        Q.sorter.wide_high = true;            // the cloud keys vary above bit 32: from 16 384 records on, wide passes there too (the one-call chain sorts 31 bits)
        SSDR_TRY(Q.sorter.sort(Q.keys.as<uint64_t>(), Q.vals.as<uint32_t>(), (int)T, nullptr, s, 64));
    }
    {
        ProfScope prof("label_scan", s, 0.0);
        hipLaunchKernelGGL(label_scan_records, dim3(1), dim3(1024), 0, s, a, (long long*)d_budget, o.class_cap, (long long*)d_out);
    }
    if (T) {
        ProfScope prof("label_apply", s, 0.0);
        hipLaunchKernelGGL(label_walk_apply_wave, dim3(grid_of(T, 4, 16)), dim3(256), 0, s, a, o);
        if (max_region == 0 || max_region > (size_t)LB_WAVE_MAX) hipLaunchKernelGGL(label_walk_apply_block, dim3(grid_of(M, 1, 4)), dim3(256), 0, s, a, o);
    }
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_oracle_label_keys_dev(const int32_t* d_picks, size_t n_picks, const int32_t* d_n_cand, const int32_t* d_cand, size_t cand_cap, const int32_t* d_gcloud, size_t Smax,
                               size_t num_gclouds, int rank, int world, const int32_t* d_cloud_key, int32_t* d_items, int32_t* d_n_items, size_t max_items, uint64_t* d_keys,
                               void* stream) {
    if (world < 1 || world > 4096 || rank < 0 || rank >= world || !d_gcloud || !d_n_items || (max_items && (!d_items || !d_keys)) || max_items > LB_MAX_ITEMS || Smax < 1 ||
        (size_t)world * Smax > 0x7ffffff0 || num_gclouds < 1 || num_gclouds > 0x7ffffff0 || n_picks > 0x7ffffff0 || cand_cap > 0x7ffffff0 ||
        (d_picks ? (!d_n_cand || !d_cand) : !d_cloud_key)) {
        set_error("oracle_label_keys: bad arguments (the picks with the candidate list, or a key per global cloud)"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); LabelState& Q = lst(s);
    ProfScope prof("label_keys", s, 0.0);
    if (d_picks) {
        SSDR_TRY(Q.first.reserve(4 * num_gclouds));
        SSDR_HIP(hipMemsetAsync(Q.first.p, 0x7f, 4 * num_gclouds, s));
        const long long G = (long long)world * (long long)Smax;
        if (n_picks) hipLaunchKernelGGL(label_pick_first, dim3(grid_of(n_picks, 256, 16)), dim3(256), 0, s, d_picks, (int)n_picks, d_n_cand, d_cand, (int)cand_cap, d_gcloud, G,
                                        (int)num_gclouds, Q.first.as<int>());
        hipLaunchKernelGGL(label_own_picks, dim3(1), dim3(1024), 0, s, d_picks, (int)n_picks, d_n_cand, d_cand, (int)cand_cap, d_gcloud, G, (int)num_gclouds,
                           (const int*)Q.first.as<int>(), rank, (int)Smax, (int)max_items, d_items, d_n_items, (unsigned long long*)d_keys);
    } else if (max_items) {
        hipLaunchKernelGGL(label_item_keys, dim3(grid_of(max_items, 256, 16)), dim3(256), 0, s, d_items, d_n_items, (int)max_items, d_gcloud, rank, (int)Smax, (int)num_gclouds,
                           d_cloud_key, (unsigned long long*)d_keys);
    }
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

}
