// mh_k_radius.h -- kernels of mh_nn_search_radius (mh_query.hip): every stored map point within a radius of each scan point,
// a VARIABLE number of results per point.  The specification is at the entry point in include/molahip.h; what pairs a point
// with a query (transform, fp32 distance, strict '<') is the un-fused arithmetic of mh_nn_device.h.
//
// Two launches of one body: k_radius<false> counts the results of every query, k_radius<true> writes them behind the exclusive
// scan of the counts.  Both run radius_walk(), so a count and a fill cannot disagree.
//
// One wave handles one query at a time.  The block of voxels that can hold a result is walked 64 voxels at a time in ascending
// (kx, ky, kz) -- the map's storage order: each lane probes one voxel's hash slot, a wave scan of the voxels' record counts
// turns the 64 runs into one numbering, and the wave then reads that numbering 64 records per step, one 16-byte record per lane
// (the runs of one column's z-neighbours are contiguous in memory on a plain map, so most steps are coalesced; an NDT map's
// statistics records sit between the runs and are never numbered).  __ballot + mbcnt give a hit its place behind the
// wave-uniform running count: results appear in storage order by construction, with no atomics, no LDS and nothing waiting
// for another workgroup.
#pragma once
#include "mh_nn_device.h"

namespace mh {

struct RadiusPose {
  double m[12];
};
struct RadiusOut {  // fill pass; any pointer may be null
  uint32_t* gi;
  float *x, *y, *z, *d2;
  unsigned long long* key;  // MH_RADIUS_SORTED: (query << 32) | bits(d2) per result
};

constexpr uint32_t kRadiusBlock = 256;  // four waves of 64

// Voxel range [lo, lo + n) of one axis that holds every stored coordinate c with a qualifying distance to p.
// d2 < r2 implies fl(dx * dx) < r2 (the fp32 sums of non-negative terms are monotone), so |c - p| < radius * (1 + 2e-7); `rr` is
// radius * 1.00001 rounded to float (host).  fl(p -+ rr) is off by at most half an ulp of the result, which 2.4e-7 * |result|
// (four half-ulps) covers; voxel_of is monotone in its argument (a rounded product by a positive constant, then floor or
// truncation), so the voxel of c lies between the voxels of the two widened ends.  With rr <= 3.00003 voxels and
// |p * inv_vs| < 1e6 the range is at most 8 voxels wide (6.0001 + 2 * 0.24 + roundings < 7 between the ends).
__device__ __forceinline__ void radius_axis(float p, float rr, float inv_vs, uint32_t trunc, int& lo, uint32_t& n) {
  float a = p - rr, b = p + rr;
  a -= fabsf(a) * 2.4e-7f;
  b += fabsf(b) * 2.4e-7f;
  lo = voxel_of(a, inv_vs, trunc);
  n = (uint32_t)(voxel_of(b, inv_vs, trunc) - lo + 1);
}

__device__ __forceinline__ uint32_t lane_rank(unsigned long long ballot) {  // set bits of `ballot` below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// The results of query (px, py, pz), in storage order; returns their number (the same in every lane).  FILL: result i goes to
// entry base + i of `o`.
template <bool FILL>
__device__ __forceinline__ uint32_t radius_walk(const MapView& m, float px, float py, float pz, float r2, float rr, uint32_t lane,
                                                uint32_t q, uint32_t base, const RadiusOut& o) {
  const float lim = 1.0e6f;  // NaN and inf fail it as well (the guard of every other search)
  if (!((int)(fabsf(px * m.inv_vs) < lim) & (int)(fabsf(py * m.inv_vs) < lim) & (int)(fabsf(pz * m.inv_vs) < lim))) return 0u;
  int lox, loy, loz;
  uint32_t nx, ny, nz;
  radius_axis(px, rr, m.inv_vs, m.trunc, lox, nx);
  radius_axis(py, rr, m.inv_vs, m.trunc, loy, ny);
  radius_axis(pz, rr, m.inv_vs, m.trunc, loz, nz);
  const uint32_t nyz = ny * nz, nvox = nx * nyz;
  const gslots_ptr slots4 = (gslots_ptr)m.slots;
  const gpts_ptr pts4 = (gpts_ptr)m.pts;
  uint32_t total = 0;
  for (uint32_t v0 = 0; v0 < nvox; v0 += 64u) {
    // 1. one voxel per lane: {first, count} of its records (count 0: absent, or outside the key range)
    uint32_t first = 0, cnt = 0;
    const uint32_t v = v0 + lane;
    if (v < nvox) {
      const uint32_t ix = v / nyz, rem = v - ix * nyz, iy = rem / nz, iz = rem - iy * nz;
      const int kx = lox + (int)ix, ky = loy + (int)iy, kz = loz + (int)iz;
      if (key_in_range(kx) && key_in_range(ky) && key_in_range(kz)) {
        const unsigned long long key = pack_key(kx, ky, kz);
        uint32_t h = hash_key(key) & m.mask;
        u32x4 sl = slots4[h];
        unsigned long long sk = ((unsigned long long)sl.y << 32) | sl.x;
        while (sk != key && sk != kEmptyKey) {  // linear probing past a collision
          h = (h + 1) & m.mask;
          sl = slots4[h];
          sk = ((unsigned long long)sl.y << 32) | sl.x;
        }
        if (sk == key) {
          first = sl.z;
          cnt = slot_count(sl.w);
        }
      }
    }
    // 2. number the records of the 64 runs: pre = records before this lane's run
    uint32_t inc = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(inc, d, 64);
      inc += lane >= (uint32_t)d ? t : 0u;
    }
    const uint32_t pre = inc - cnt;
    const uint32_t run_total = __shfl(inc, 63, 64);
    // 3. 64 records per step, one per lane
    for (uint32_t t0 = 0; t0 < run_total; t0 += 64u) {
      const uint32_t t = t0 + lane;
      const bool valid = t < run_total;
      // the run of record t: the last lane j with pre[j] <= t (runs of count 0 share their successor's pre and lose to it)
      uint32_t j = 0, pj = __shfl(pre, 0, 64);
#pragma unroll
      for (int b = 32; b > 0; b >>= 1) {
        const uint32_t pv = __shfl(pre, (int)(j + (uint32_t)b), 64);
        const bool take = pv <= t;
        j = take ? j + (uint32_t)b : j;
        pj = take ? pv : pj;
      }
      const uint32_t fj = __shfl(first, (int)j, 64);
      bool hit = false;
      f32x4 c = (f32x4)(0.f);
      float d2 = 0.f;
      if (valid) {
        c = pts4[fj + (t - pj)];
        const float dx = c.x - px, dy = c.y - py, dz = c.z - pz;
        d2 = (dx * dx + dy * dy) + dz * dz;  // fp32, un-fused, this order (bit-exact with the oracle)
        hit = d2 < r2;
      }
      const unsigned long long hits = __ballot(hit);
      if (FILL && hit) {
        const size_t e = (size_t)base + total + lane_rank(hits);
        if (o.gi) o.gi[e] = __float_as_uint(c.w);
        if (o.x) o.x[e] = c.x;
        if (o.y) o.y[e] = c.y;
        if (o.z) o.z[e] = c.z;
        if (o.d2) o.d2[e] = d2;
        if (o.key) o.key[e] = ((unsigned long long)q << 32) | __float_as_uint(d2);
      }
      total += (uint32_t)__popcll(hits);
    }
  }
  return total;
}

// FILL = false: counts[q] = results of query q.  FILL = true: the results of query q at entries [offsets[q], offsets[q + 1]).
template <bool FILL>
__global__ __launch_bounds__(kRadiusBlock) void k_radius(RadiusPose T, float r2, float rr, const float* __restrict__ x,
                                                         const float* __restrict__ y, const float* __restrict__ z, uint32_t n,
                                                         MapView m, uint32_t* __restrict__ counts,
                                                         const uint32_t* __restrict__ offsets, RadiusOut o) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n_waves = gridDim.x * (kRadiusBlock / 64u);
  for (uint32_t q = blockIdx.x * (kRadiusBlock / 64u) + (threadIdx.x >> 6); q < n; q += n_waves) {
    float px, py, pz;
    transform_point(T.m, x[q], y[q], z[q], px, py, pz);
    const uint32_t base = FILL ? offsets[q] : 0u;
    const uint32_t total = radius_walk<FILL>(m, px, py, pz, r2, rr, lane, q, base, o);
    if (!FILL && lane == 0) counts[q] = total;
  }
}

// stats[0..1] (64 bits) += sum of counts, stats[2] = max of counts; both zeroed by the caller
__global__ __launch_bounds__(kRadiusBlock) void k_radius_stats(const uint32_t* __restrict__ counts, uint32_t n,
                                                               unsigned long long* __restrict__ sum, uint32_t* __restrict__ mx) {
  unsigned long long s = 0;
  uint32_t m = 0;
  for (uint32_t i = blockIdx.x * kRadiusBlock + threadIdx.x; i < n; i += gridDim.x * kRadiusBlock) {
    const uint32_t c = counts[i];
    s += c;
    m = c > m ? c : m;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    s += __shfl_xor(s, d, 64);
    const uint32_t om = __shfl_xor(m, d, 64);
    m = om > m ? om : m;
  }
  if ((threadIdx.x & 63u) == 0) {
    if (s) atomicAdd(sum, s);
    if (m) atomicMax(mx, m);
  }
}

// MH_RADIUS_SORTED: entry e of the outputs = entry perm[e] of the storage-order results
__global__ __launch_bounds__(kRadiusBlock) void k_radius_gather(const uint32_t* __restrict__ perm, size_t n, RadiusOut src,
                                                                RadiusOut dst) {
  const size_t e = (size_t)blockIdx.x * kRadiusBlock + threadIdx.x;
  if (e >= n) return;
  const uint32_t p = perm[e];
  if (dst.gi) dst.gi[e] = src.gi[p];
  if (dst.x) dst.x[e] = src.x[p];
  if (dst.y) dst.y[e] = src.y[p];
  if (dst.z) dst.z[e] = src.z[p];
  if (dst.d2) dst.d2[e] = src.d2[p];
}

}  // namespace mh
