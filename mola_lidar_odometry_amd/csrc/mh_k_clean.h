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
// The tables are kernel arguments (wave-uniform: scalar loads).  All point arithmetic is un-fused fp32 (-ffp-contract=off).
#pragma once
#include <stdint.h>

#include "mh_place_bin.h"
#include "mh_nn_device.h"

namespace mh {

constexpr uint32_t kCleanBlock = 256;  // four waves of 64

struct CleanTables {  // built on the host in fp64, rounded once (clean_make_tables, mh_clean.hip)
  float tan_edge[MH_CLEAN_MAX_SECTORS / 8];  // [0] unused: j = 1 .. S/8-1
  float el_tan2[MH_CLEAN_MAX_RINGS + 1];
  int32_t el_sign[MH_CLEAN_MAX_RINGS + 1];
  float min_r2, max_r2, far2;
  float ox, oy, oz;
  uint32_t A, S, win_rings, win_sectors;
};

// "elevation edge k lies at or below the point"
__device__ __forceinline__ bool clean_above(const CleanTables& t, uint32_t k, float h2, float z, float zz) {
  const float m = t.el_tan2[k] * h2;
  const int32_t s = t.el_sign[k];
  if (s > 0) return z > 0.f && zz >= m;
  if (s == 0) return z >= 0.f;
  return z >= 0.f || zz <= m;
}

// ring, sector and squared range of a point given in the vehicle frame; false: the point is skipped
__device__ __forceinline__ bool clean_bin(const CleanTables& t, float px, float py, float pz, uint32_t& ring, uint32_t& sector,
                                          float& r2) {
  const float x = px - t.ox, y = py - t.oy, z = pz - t.oz;
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  if (x == 0.f && y == 0.f) return false;
  const float h2 = x * x + y * y, zz = z * z;
  r2 = h2 + zz;
  if (!(r2 >= t.min_r2 && r2 < t.max_r2)) return false;
  if (!clean_above(t, 0u, h2, z, zz) || clean_above(t, t.A, h2, z, zz)) return false;
  ring = 0;
  for (uint32_t k = 1; k < t.A; k++) ring += clean_above(t, k, h2, z, zz) ? 1u : 0u;
  sector = place_sector(t.tan_edge, t.S, x, y);
  return true;
}

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
    for (uint32_t i = threadIdx.x; i < AS; i += kPlaceBlock) sh_bins[i] = MH_CLEAN_EMPTY;
    __syncthreads();
    const float* __restrict__ fx = fr[f].x;
    const float* __restrict__ fy = fr[f].y;
    const float* __restrict__ fz = fr[f].z;
    const uint32_t base = start[f];
    for (uint32_t q = lo + threadIdx.x; q < hi; q += kPlaceBlock) {
      const uint32_t j = q - base;
      uint32_t ring, sector;
      float r2;
      if (clean_bin(tab, fx[j], fy[j], fz[j], ring, sector, r2)) atomicMin(&sh_bins[ring * tab.S + sector], __float_as_uint(r2));
    }
    __syncthreads();
    uint32_t* __restrict__ out = views + (size_t)f * AS;
    for (uint32_t i = threadIdx.x; i < AS; i += kPlaceBlock) {
      const uint32_t v = sh_bins[i];
      if (v != MH_CLEAN_EMPTY) atomicMin(&out[i], v);
    }
    __syncthreads();  // (the bins are preset again for the next frame)
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
  const int32_t wr = (int32_t)tab.win_rings, ws = (int32_t)tab.win_sectors;
  uint32_t through = 0, agree = 0;
  typedef const double __attribute__((address_space(4))) * cf64_ptr;
  const uint32_t k1 = nbr_start[f + 1u];
  for (uint32_t k = nbr_start[f]; k < k1; k++) {  // (uniform)
    const cf64_ptr Tp = (cf64_ptr)uniform_const_ptr(nbr_T + 12 * (size_t)k);
    double T[12];
#pragma unroll
    for (int e = 0; e < 12; e++) T[e] = Tp[e];
    const uint32_t* __restrict__ view = views + (size_t)nbr_view[k] * AS;
    float qx, qy, qz, r2q;
    transform_point(T, px, py, pz, qx, qy, qz);
    uint32_t ring, sector;
    if (!clean_bin(tab, qx, qy, qz, ring, sector, r2q)) continue;
    const float lim = r2q * tab.far2;
    const uint32_t own = view[ring * tab.S + sector];
    if (own == MH_CLEAN_EMPTY) continue;
    const float r2o = __uint_as_float(own);
    if (r2o > lim) {  // through, unless a bin of the window is empty or not farther
      bool all_far = true;
      for (int32_t dr = -wr; dr <= wr; dr++) {
        const int32_t rr = (int32_t)ring + dr;
        if (rr < 0 || rr >= (int32_t)tab.A) continue;
        for (int32_t ds = -ws; ds <= ws; ds++) {
          int32_t ss = (int32_t)sector + ds;
          ss = ss < 0 ? ss + (int32_t)tab.S : (ss >= (int32_t)tab.S ? ss - (int32_t)tab.S : ss);
          const uint32_t w = view[(uint32_t)rr * tab.S + (uint32_t)ss];
          all_far = all_far && w != MH_CLEAN_EMPTY && __uint_as_float(w) > lim;
        }
      }
      if (all_far) through += through < 65535u ? 1u : 0u;
    } else if (r2q <= r2o * tab.far2) {  // (r2o <= r2q * far2 holds on this branch)
      agree += agree < 65535u ? 1u : 0u;
    }
  }
  votes[base + i] = through | agree << 16;
}

}  // namespace mh
