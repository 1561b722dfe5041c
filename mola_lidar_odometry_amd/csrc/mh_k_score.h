// mh_k_score.h -- the kernel of mh_score_poses (mh_query.hip): one scan against one map under MANY candidate poses, one launch.
// The specification is at the entry point in include/molahip.h; what pairs a point (transform, fp32 distance, first strict
// minimum, acceptance test) is the un-fused arithmetic of mh_nn_device.h and of k_match.
//
// One workgroup of 256 lanes = one candidate x one tile of 256 scan points; the grid is flat (candidate * n_tiles + tile:
// gridDim.y stops at 65535 and the candidate count does not).  The pose is wave-uniform and comes through scalar loads; lane =
// point, coalesced SoA reads.  The search is nn_search_pruned started from the ACCEPTANCE bound instead of +inf: a neighbour at
// or beyond the bound is rejected anyway, so the accepted set and every accepted d2 are those of the unbounded search, and
// most neighbour voxels of a wrong candidate are never probed.  Scores are integers: wave reduction by shuffles, the four
// waves through LDS, then one pair of integer atomics per workgroup into the zeroed score of its candidate -- exact and
// independent of the order of arrival.
#pragma once
#include "mh_nn_device.h"

namespace mh {

constexpr uint32_t kScoreBlock = 256;  // four waves of 64

// nn_search_pruned with the best distance starting at `bound`: true iff the 27-voxel block holds a record with d2 < bound, and
// then d2 is mh_nn_search_dense's (the minimum; which of several records at that distance wins does not enter a score).
// A voxel is skipped only when its conservative lower bound exceeds the best so far (<= bound), so every record with
// d2 < bound is seen.  A record at exactly d2 == bound may be taken as the best (record index < "none") and is then not accepted.
__device__ __forceinline__ bool nn_search_within(const MapView& m, float qx, float qy, float qz, float bound, float& d2) {
  const int cx = voxel_of(qx, m.inv_vs, m.trunc), cy = voxel_of(qy, m.inv_vs, m.trunc), cz = voxel_of(qz, m.inv_vs, m.trunc);
  const unsigned long long kbase = pack_key(cx - 1, cy - 1, cz - 1);
  const gslots_ptr slots4 = (gslots_ptr)m.slots;
  const gpts_ptr pts4 = (gpts_ptr)m.pts;
  const Gaps gx = axis_gaps(qx, cx, m.vs, m.trunc), gy = axis_gaps(qy, cy, m.vs, m.trunc), gz = axis_gaps(qz, cz, m.vs, m.trunc);
  NNBest b;
  b.d2 = bound;
  b.idx = 0xFFFFFFFFu;
  {  // the query's own voxel (code 13)
    const unsigned long long key = nn_key_of(kbase, 13);
    nn_visit(m, slots4, pts4, key, slots4[hash_key(key) & m.mask], qx, qy, qz, b);
  }
  uint32_t mask = 0;
#pragma unroll
  for (int c = 0; c < 27; c++) {
    if (c == 13) continue;
    const float lb = (gx.s[c / 9] + gy.s[(c / 3) % 3]) + gz.s[c % 3];
    if (!(lb * 0.9999f > b.d2)) mask |= 1u << c;
  }
  // faces, edges, corners: nearer voxels tighten the bound for the farther ones (nn_search_pruned's order)
  const uint32_t kFaces = (1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22);
  const uint32_t kCorners = (1u << 0) | (1u << 2) | (1u << 6) | (1u << 8) | (1u << 18) | (1u << 20) | (1u << 24) | (1u << 26);
  const uint32_t kEdges = 0x07FFFFFFu & ~(kFaces | kCorners | (1u << 13));
#pragma unroll 1
  for (int cls = 0; cls < 3; cls++) {
    uint32_t mm = mask & (cls == 0 ? kFaces : (cls == 1 ? kEdges : kCorners));
    while (mm) {
      const int c = __builtin_ctz(mm);
      mm &= mm - 1;
      if (nn_lower_bound(c, gx, gy, gz) * 0.9999f > b.d2) continue;
      const unsigned long long key = nn_key_of(kbase, c);
      nn_visit(m, slots4, pts4, key, slots4[hash_key(key) & m.mask], qx, qy, qz, b);
    }
  }
  d2 = b.d2;
  return b.idx != 0xFFFFFFFFu && b.d2 < bound;
}

// scores[c] += {accepted points, sum of their quantised d2} of tile (blockIdx.x % n_tiles) under pose c = blockIdx.x / n_tiles;
// the caller has zeroed `scores`
__global__ __launch_bounds__(kScoreBlock) void k_score_poses(const double* __restrict__ poses, uint32_t n_tiles,
                                                             const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ z, uint32_t n, MapView map, float thr2,
                                                             float ang2, float qscale, mh_pose_score* __restrict__ scores) {
  __shared__ uint32_t sh_n[kScoreBlock / 64];
  __shared__ unsigned long long sh_c[kScoreBlock / 64];
  const uint32_t c = blockIdx.x / n_tiles, tile = blockIdx.x - c * n_tiles;  // (uniform)
  typedef const double __attribute__((address_space(4))) * cf64_ptr;
  const cf64_ptr Tp = (cf64_ptr)uniform_const_ptr(poses + 12 * (size_t)c);
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; i++) T[i] = Tp[i];
  const uint32_t i = tile * kScoreBlock + threadIdx.x;
  uint32_t np = 0;
  unsigned long long cost = 0;
  if (i < n) {  // (lanes past the end contribute zeros and still reach the reduction below)
    float px, py, pz;
    transform_point(T, x[i], y[i], z[i], px, py, pz);
    const float lim = 1.0e6f;  // NaN and inf fail it as well (the guard of every other search)
    if ((int)(fabsf(px * map.inv_vs) < lim) & (int)(fabsf(py * map.inv_vs) < lim) & (int)(fabsf(pz * map.inv_vs) < lim)) {
      const float n2 = (px * px + py * py) + pz * pz;
      const float bound = thr2 + ang2 * n2;  // mh_nn_search's acceptance: d2 < thr2 + ang2 * |p'|^2
      float d2;
      if (nn_search_within(map, px, py, pz, bound, d2)) {
        const float qs = d2 * qscale;
        np = 1u;
        cost = (qs >= 16777215.0f) ? 0xFFFFFFull : (unsigned long long)(uint32_t)qs;
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    np += __shfl_xor(np, d, 64);
    cost += __shfl_xor(cost, d, 64);
  }
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
    sh_n[w] = np;
    sh_c[w] = cost;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tn = 0;
    unsigned long long tc = 0;
#pragma unroll
    for (uint32_t q = 0; q < kScoreBlock / 64; q++) {
      tn += sh_n[q];
      tc += sh_c[q];
    }
    if (tn) {  // (cost > 0 implies a pair)
      atomicAdd(&scores[c].n_paired, tn);
      atomicAdd((unsigned long long*)&scores[c].cost, tc);
    }
  }
}

}  // namespace mh
