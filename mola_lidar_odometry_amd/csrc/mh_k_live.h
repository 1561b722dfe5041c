// mh_k_live.h -- see-through voting on the stored records of a live map and the erasing of flagged points (included by
// mh_live.hip; the specification is the text of include/molahip_live.h, THE RULE that of include/molahip_clean.h).  Binning,
// view accumulation and the vote are mh_see_through.h's, shared with mh_k_clean.h.  Kernels:
//   k_view_put:      the view of one device-resident scan: k_view_build's workgroup (kPlaceChunk consecutive points, bins in
//                    LDS, touched bins flushed with a global atomicMin) without the frame search.
//   k_vote_map:      one lane per stored 16-byte record (one dwordx4, coalesced), 256-lane workgroups.  The neighbour table of
//                    the launch (view index and twelve doubles per entry) is a kernel argument: uniform, read through scalar
//                    loads like the tables.  Window words are gathered from global memory; two counters per lane in registers;
//                    one packed word per record out with an ordinary store; no atomics, no LDS, no barrier.  A neighbour list
//                    longer than kLiveLaunchViews takes further launches that add, saturating, to the words of the one before.
//                    The two statistics records in front of an NDT voxel's points are voted on like points; nobody reads their
//                    words.
//   k_live_keep:     one lane per voxel: keep[i] = 0 / 1 for every stored point i (download order) from the vote words of its
//                    records and the decision rule, or from the caller's drop bytes.
//   k_live_pick:     one lane per voxel: the words of a voxel's point records into download order (NDT maps only: elsewhere the
//                    record order is the download order).
//   k_live_compact:  the kept points, in order, to the front of the rebuild's input arrays (positions from an exclusive scan of
//                    keep); the places behind them get a point without a key (NaN), which every rebuild sorts last and skips.
// An erasing may be queued behind an update whose counts the host has not seen yet: the grids then cover the host's bounds, and
// every kernel takes the true voxel and record counts from the device counters of that update (`counters`: [0] its out-of-range
// flag, [9] voxels, [10] records), as k_ndt_stats and k_table_insert do.
#pragma once
#include <stdint.h>

#include "mh_see_through.h"

namespace mh {

constexpr uint32_t kLiveBlock = 256;       // four waves of 64
constexpr uint32_t kLiveLaunchViews = 24;  // neighbour entries per launch: 2.4 KB of kernel arguments

struct LiveNbr {
  double T[kLiveLaunchViews][12];
  uint32_t view[kLiveLaunchViews];
};

// view[bin] = min(.., bits of r2) over the scan's points; the caller has preset `view` [A*S] to empty
__global__ __launch_bounds__(kPlaceBlock) void k_view_put(const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ z, uint32_t n, CleanTables tab,
                                                          uint32_t* __restrict__ view) {
  __shared__ uint32_t sh_bins[MH_CLEAN_MAX_BINS];
  const uint32_t q0 = blockIdx.x * kPlaceChunk;  // (uniform; the grid covers n: q0 < n)
  view_accumulate(sh_bins, tab, x, y, z, q0, min(q0 + kPlaceChunk, n), view);
}

// votes[r] (+)= through | agree << 16 of record r against the n_nb views of `nb`
__global__ __launch_bounds__(kLiveBlock) void k_vote_map(const float4* __restrict__ pts, const uint32_t* __restrict__ counters,
                                                         LiveNbr nb, uint32_t n_nb, const uint32_t* __restrict__ views,
                                                         CleanTables tab, uint32_t add, uint32_t* __restrict__ votes) {
  const uint32_t r = blockIdx.x * kLiveBlock + threadIdx.x;
  if (r >= counters[10]) return;  // (the grid covers the host's bound of the record count; no barrier below)
  const float4 p = pts[r];
  const uint32_t AS = tab.A * tab.S;
  uint32_t through = 0, agree = 0;
  for (uint32_t k = 0; k < n_nb; k++) {  // (uniform)
    double T[12];
#pragma unroll
    for (int e = 0; e < 12; e++) T[e] = nb.T[k][e];
    see_through_vote(tab, views + (size_t)nb.view[k] * AS, T, p.x, p.y, p.z, through, agree);
  }
  if (add) {
    const uint32_t before = votes[r];
    through = min((before & 0xFFFFu) + through, 65535u);
    agree = min((before >> 16) + agree, 65535u);
  }
  votes[r] = through | agree << 16;
}

// first point of voxel v in the point-only numbering of a download
__device__ __forceinline__ uint32_t live_download_pos(uint32_t first, uint32_t v, uint32_t ndt) {
  return ndt ? first - 2u * (v + 1u) : first;
}

// (the caller has preset keep [the host's bound of the point count] to 0: what lies behind the stored points is not kept)
__global__ void k_live_keep(const uint32_t* __restrict__ vox_first, const uint32_t* __restrict__ vox_count,
                            const uint32_t* __restrict__ counters, uint32_t ndt,
                            const uint32_t* __restrict__ votes /* per record, or null */, uint32_t min_through_votes,
                            uint32_t agree_weight, const uint8_t* __restrict__ drop /* per point */, uint32_t* __restrict__ keep) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= counters[9]) return;
  const uint32_t first = vox_first[v], cnt = vox_count[v];
  const uint32_t o = live_download_pos(first, v, ndt);
  for (uint32_t j = 0; j < cnt; j++) {
    bool gone;
    if (votes) {
      const uint32_t w = votes[first + j], th = w & 0xFFFFu, ag = w >> 16;
      gone = th >= min_through_votes && (unsigned long long)th > (unsigned long long)agree_weight * ag;
    } else {
      gone = drop[o + j] != 0;
    }
    keep[o + j] = gone ? 0u : 1u;
  }
}

__global__ void k_live_pick(const uint32_t* __restrict__ vox_first, const uint32_t* __restrict__ vox_count,
                            const uint32_t* __restrict__ counters, const uint32_t* __restrict__ votes, uint32_t* __restrict__ out) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= counters[9]) return;
  const uint32_t first = vox_first[v], cnt = vox_count[v];
  const uint32_t o = live_download_pos(first, v, 1u);
  for (uint32_t j = 0; j < cnt; j++) out[o + j] = votes[first + j];
}

struct LiveCarry {  // mh_map::d_live
  unsigned long long erased;  // points erased since the map was created
  unsigned long long flag;    // != 0: an update whose counters this rebuild overwrites held out-of-range points
};

// (the grid covers n, the host's bound of the point count; a map holds no more voxels than points)
__global__ void k_live_compact(const float4* __restrict__ pts, const uint32_t* __restrict__ vox_first,
                               const uint32_t* __restrict__ vox_count, const uint32_t* __restrict__ counters, uint32_t ndt,
                               const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos, uint32_t n, uint32_t carry_flag,
                               LiveCarry* __restrict__ carry, float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz,
                               uint32_t* __restrict__ osrc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n_kept = pos[n - 1u] + keep[n - 1u];
  const uint32_t n_vox = counters[9];
  if (i == 0) {  // (one lane of the launch; launches of one map are ordered on its stream)
    carry->erased += (counters[10] - (ndt ? 2u * n_vox : 0u)) - n_kept;
    if (carry_flag && (counters[0] & 1u)) carry->flag = 1ull;
  }
  if (i < n && i >= n_kept) {  // behind the kept points: no key
    ox[i] = __uint_as_float(0x7FC00000u);
    oy[i] = 0.f;
    oz[i] = 0.f;
    osrc[i] = 0u;
  }
  if (i >= n_vox) return;
  const uint32_t first = vox_first[i], cnt = vox_count[i];
  const uint32_t o = live_download_pos(first, i, ndt);
  for (uint32_t j = 0; j < cnt; j++) {
    if (!keep[o + j]) continue;
    const uint32_t d = pos[o + j];  // (< n_kept)
    const float4 p = pts[first + j];
    ox[d] = p.x;
    oy[d] = p.y;
    oz[d] = p.z;
    osrc[d] = __float_as_uint(p.w);
  }
}

}  // namespace mh
