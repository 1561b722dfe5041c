// mh_see_through.h -- what the see-through kernels share: the host-built tables, the binning of a point, the accumulation of
// one frame's points into a view and the vote of one point against one view (the specification is the text of
// include/molahip_clean.h).  Included by mh_k_clean.h (key-frames) and mh_k_live.h (a live map); device functions only, no
// kernel.  All point arithmetic is un-fused fp32 (-ffp-contract=off).
#pragma once
#include <stdint.h>

#include "../../include/molahip_clean.h"
#include "mh_place_bin.h"
#include "mh_nn_device.h"

namespace mh {

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

// One workgroup of kPlaceBlock lanes takes the points j = lo .. hi-1 of one frame (fx, fy, fz) into that frame's view `out`
// [A * S], preset to empty by the caller: A*S words in LDS preset to "empty", the minimum squared range per bin with atomicMin
// in LDS, only the touched bins flushed with a global atomicMin.  Every lane of the workgroup calls it (barriers inside); the
// bins are free again on return.
__device__ __forceinline__ void view_accumulate(uint32_t* sh_bins, const CleanTables& tab, const float* __restrict__ fx,
                                                const float* __restrict__ fy, const float* __restrict__ fz, uint32_t lo,
                                                uint32_t hi, uint32_t* __restrict__ out) {
  const uint32_t AS = tab.A * tab.S;
  for (uint32_t i = threadIdx.x; i < AS; i += kPlaceBlock) sh_bins[i] = MH_CLEAN_EMPTY;
  __syncthreads();
  for (uint32_t j = lo + threadIdx.x; j < hi; j += kPlaceBlock) {
    uint32_t ring, sector;
    float r2;
    if (clean_bin(tab, fx[j], fy[j], fz[j], ring, sector, r2)) atomicMin(&sh_bins[ring * tab.S + sector], __float_as_uint(r2));
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < AS; i += kPlaceBlock) {
    const uint32_t v = sh_bins[i];
    if (v != MH_CLEAN_EMPTY) atomicMin(&out[i], v);
  }
  __syncthreads();  // (the bins are preset again for the next frame)
}

// THE VOTE of one point against one view under T (twelve doubles, row-major 3x4): the point's counters go up, saturating.  The
// view's words are gathered from global memory (a view is at most 16 KB and stays in L2; the own bin is read first and decides
// whether the rest of the window is read at all).
__device__ __forceinline__ void see_through_vote(const CleanTables& tab, const uint32_t* __restrict__ view, const double T[12],
                                                 float px, float py, float pz, uint32_t& through, uint32_t& agree) {
  const int32_t wr = (int32_t)tab.win_rings, ws = (int32_t)tab.win_sectors;
  float qx, qy, qz, r2q;
  transform_point(T, px, py, pz, qx, qy, qz);
  uint32_t ring, sector;
  if (!clean_bin(tab, qx, qy, qz, ring, sector, r2q)) return;
  const float lim = r2q * tab.far2;
  const uint32_t own = view[ring * tab.S + sector];
  if (own == MH_CLEAN_EMPTY) return;
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

}  // namespace mh
