// mh_k_clean.h -- see-through voting on key-frame views (included by mh_clean.hip; the specification is the text of
// include/molahip_clean.h).  Two kernels:
//   k_view_build:  one lane per point of a whole pass of frames, the shape of k_place_describe: a workgroup owns kPlaceChunk
//                  consecutive points, finds their frames by wave-uniform upper-bound searches in the prefix array, keeps A*S words
//                  in LDS (at most 16 KB) preset to "empty", takes the minimum squared range per bin with atomicMin in LDS and
//                  flushes only the touched bins with a global atomicMin into the frame's preset view.  Positive floats order as
//                  unsigned integers: exact whatever the arrival order.
//   k_see_through: one workgroup per (frame, tile of 256 points), lane = point.  The workgroup walks the frame's neighbour list;
//                  list, view index and pose are uniform across the workgroup and come through scalar loads (as k_score_poses'
//                  pose).  Each lane projects its point, bins it and gathers the window words of the neighbour's view from
//                  global memory (a view is at most 16 KB and stays in L2; the own bin is read first and decides whether the
//                  rest of the window is read at all).  Two counters per lane in registers, one packed word per point out; no
//                  atomics, no LDS, no barrier.
// The tables are kernel arguments (wave-uniform: scalar loads).  Binning, view accumulation and the vote itself are
// mh_see_through.h's, shared with the kernels of a live map (mh_k_live.h).
#pragma once
#include <stdint.h>

#include "mh_see_through.h"

namespace mh {

constexpr uint32_t kCleanBlock = 256;  // four waves of 64

// views[f * A*S + bin] = min(.., bits of r2) over the points of frame f; the caller has preset `views` [n_frames * A*S] to empty
__global__ __launch_bounds__(kPlaceBlock) void k_view_build(const uint32_t* __restrict__ start, const PlaceSrc* __restrict__ fr,
                                                            uint32_t n_frames, uint32_t total, CleanTables tab,
                                                            uint32_t* __restrict__ views) {
  __shared__ uint32_t sh_bins[MH_CLEAN_MAX_BINS];
  const uint32_t q0 = blockIdx.x * kPlaceChunk;  // (uniform; the grid covers `total`: q0 < total)
  const uint32_t q1 = min(q0 + kPlaceChunk, total);
  const uint32_t AS = tab.A * tab.S;
  const uint32_t f_first = place_frame_of(start, 0u, n_frames - 1u, q0);
  const uint32_t f_last = place_frame_of(start, f_first, n_frames - 1u, q1 - 1u);
  for (uint32_t f = f_first; f <= f_last; f++) {  // (uniform trip count)
    const uint32_t lo = max(start[f], q0), hi = min(start[f + 1u], q1);
    if (lo >= hi) continue;  // (an empty frame between two others; uniform)
    const uint32_t base = start[f];
    view_accumulate(sh_bins, tab, fr[f].x, fr[f].y, fr[f].z, lo - base, hi - base, views + (size_t)f * AS);
  }
}

// votes[pt_start[f] + i] = through | agree << 16 of point i of frame f against the views of its neighbour list.  Workgroup b serves
// tile b - tile_start[f] of the frame f found by the upper-bound search in tile_start (frames without points own no tile).
__global__ __launch_bounds__(kCleanBlock) void k_see_through(const uint32_t* __restrict__ tile_start,
                                                             const uint32_t* __restrict__ pt_start, const PlaceSrc* __restrict__ fr,
                                                             uint32_t n_frames, const uint32_t* __restrict__ nbr_start,
                                                             const uint32_t* __restrict__ nbr_view, const double* __restrict__ nbr_T,
                                                             const uint32_t* __restrict__ views, CleanTables tab,
                                                             uint32_t* __restrict__ votes) {
  const uint32_t f = place_frame_of(tile_start, 0u, n_frames - 1u, blockIdx.x);  // (uniform)
  const uint32_t base = pt_start[f], n = pt_start[f + 1u] - base;
  const uint32_t i = (blockIdx.x - tile_start[f]) * kCleanBlock + threadIdx.x;
  if (i >= n) return;  // (no barrier below)
  const float px = fr[f].x[i], py = fr[f].y[i], pz = fr[f].z[i];
  const uint32_t AS = tab.A * tab.S;
  uint32_t through = 0, agree = 0;
  typedef const double __attribute__((address_space(4))) * cf64_ptr;
  const uint32_t k1 = nbr_start[f + 1u];
  for (uint32_t k = nbr_start[f]; k < k1; k++) {  // (uniform)
    const cf64_ptr Tp = (cf64_ptr)uniform_const_ptr(nbr_T + 12 * (size_t)k);
    double T[12];
#pragma unroll
    for (int e = 0; e < 12; e++) T[e] = Tp[e];
    see_through_vote(tab, views + (size_t)nbr_view[k] * AS, T, px, py, pz, through, agree);
  }
  votes[base + i] = through | agree << 16;
}

}  // namespace mh
