// mh_place_bin.h -- what the polar binning kernels share: the flat-pass geometry (a workgroup owns a chunk of consecutive points
// of a pass of frames), the frame search in the prefix array and the sector rule of mh_place_describe.  Included by
// mh_k_place.h (descriptors) and mh_k_clean.h (view images); device functions only, no kernel.
#pragma once
#include <stdint.h>

namespace mh {

constexpr uint32_t kPlaceBlock = 256;                // four waves of 64
constexpr uint32_t kPlacePointsPerLane = 8;
constexpr uint32_t kPlaceChunk = kPlaceBlock * kPlacePointsPerLane;  // points of a pass per workgroup

struct PlaceSrc {
  const float *x, *y, *z;  // the frame's points (device memory; never read for an empty frame)
};

// the frame of point q: the last f in [lo, hi] with start[f] <= q; empty frames are stepped over by the upper bound
__device__ __forceinline__ uint32_t place_frame_of(const uint32_t* __restrict__ start, uint32_t lo, uint32_t hi, uint32_t q) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (start[mid] <= q) lo = mid;
    else hi = mid - 1u;
  }
  return lo;
}

// the sector (0..S-1) of a finite (x, y) other than (0, 0): quarter turns, then the tan_edge table [S/8] of the specification
__device__ __forceinline__ uint32_t place_sector(const float* tan_edge, uint32_t S, float x, float y) {
  uint32_t Q;
  float a, b;
  if (x > 0.f && y >= 0.f) { Q = 0; a = x; b = y; }
  else if (x <= 0.f && y > 0.f) { Q = 1; a = y; b = -x; }
  else if (x < 0.f && y <= 0.f) { Q = 2; a = -x; b = -y; }
  else { Q = 3; a = -y; b = x; }
  const uint32_t E = S >> 3;
  uint32_t o = 0;
  if (b < a) {
    for (uint32_t j = 1; j < E; j++) o += b >= tan_edge[j] * a ? 1u : 0u;
  } else {
    for (uint32_t j = 1; j < E; j++) o += a > tan_edge[j] * b ? 1u : 0u;
    o = (2u * E - 1u) - o;
  }
  return Q * (S >> 2) + o;
}

}  // namespace mh
