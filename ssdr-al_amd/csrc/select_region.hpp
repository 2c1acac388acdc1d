// The region selectors beside gcn_fps (select_region.hip): what select.hip's one-call chains need of them.
#pragma once
#include "ssdr_internal.hpp"

namespace ssdr {

constexpr int EDCD_MAX_ROWS = 8192;       // candidates of one cloud the edcd FPS takes (its running minima live in LDS), as ssdr_fps_superpoint_dev

// status bits of the edcd chain (OR-ed into the word *d_status; bits 0-1 belong to the candidate rule, cand_layout)
constexpr int EDCD_ST_TOO_BIG = 4;        // a cloud has more than EDCD_MAX_ROWS candidates (or more than n_max)
constexpr int EDCD_ST_COUNT = 8;          // a cloud asks for more picks than it has candidates
constexpr int EDCD_ST_CAP = 16;           // the picks of all clouds exceed max_select

// farthest_superpoint_sample of every cloud in one launch, enqueued: cloud b's rows are d_coff[b] .. d_coff[b+1]-1 (centres [rows, 3]), its directed
// chamfer means the n_b x n_b block at d_boff[b] of d_cd_dir — symmetrised in place (dir + dir^T, diagonal 0) — and it picks d_ntop[b] of them from its
// first row; the picks (row indices) land at the exclusive prefix of d_ntop.  Nothing runs while *d_status != 0 (a status the candidate rule set is
// respected); d_ooff [num_clouds + 1] is scratch.  n_max: bound on n_b the LDS is sized by (clouds above min(n_max, EDCD_MAX_ROWS) set EDCD_ST_TOO_BIG).
int edcd_fps_launch(const double* d_centres, double* d_cd_dir, const int* d_coff, const long long* d_boff, const int* d_ntop, int num_clouds, int n_max,
                    long long max_select, int* d_ooff, int* d_status, int* d_out, hipStream_t s);

}  // namespace ssdr
