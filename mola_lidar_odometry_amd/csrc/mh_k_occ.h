// mh_k_occ.h -- kernel bodies of the occupancy voxel map (mh_occmap.hip; the reading is written down in include/molahip.h).
//
// An insert is restated data-parallel with no cross-thread waiting and no float atomics:
//   k_occ_rays     per point: compose with the pose, the three tests, end cell, number of work items of its ray
//   (prefix sum over the items)
//   k_occ_keys     per WORK ITEM (ray, step): one 64-bit key  cell << 1 | is_miss  -- the hot path
//   (sort, run-length encode: per (cell, kind) counts; passes are merged and summed by key)
//   k_occ_cells    (cell, kind) entries -> one (cell, h, m) entry per touched cell
//   k_occ_join     which touched cells are new to the store (binary search, the store is sorted)
//   k_occ_merge    store and new cells into one sorted sequence, the update rule applied, keep / occupied flags
//   (prefix sum over the flags)
//   k_occ_compact  far removal: the kept cells into the other store buffer, the occupied centres into a point layer
#pragma once
#include "mh_internal.h"

// (the kernels are static: mh_occmap.hip and mh_occgrid.hip both include this file)

namespace mh {
namespace occ {

struct Pose12 { double m[12]; };

// the five integers the device sees (mh_occmap_info) and the rule
struct Rule {
  int l_hit, l_miss, l_min, l_max, l_occ;
  uint32_t once;  // MH_OCC_ONCE
};

__device__ __forceinline__ int cell_index(float c, float inv_res, uint32_t trunc) {
  const float s = c * inv_res;  // fp32 product, un-fused (the key rule of mh_map)
  return trunc ? (int)s : (int)floorf(s);
}

// remove_voxels_farther_than's index distance test (mh_map_params::far_voxel_metric), the rule of mh_map_insert
__device__ __forceinline__ bool far_cell(int dx, int dy, int dz, int dist, uint32_t metric) {
  dx = abs(dx); dy = abs(dy); dz = abs(dz);
  if (metric == MH_FAR_L1) return (long long)dx + dy + dz > (long long)dist;
  if (metric == MH_FAR_L2) return (long long)dx * dx + (long long)dy * dy + (long long)dz * dz > (long long)dist * dist;
  return max(max(dx, dy), dz) > dist;
}

__device__ __forceinline__ int apply_rule(int l, uint32_t h, uint32_t m, const Rule& r) {
  long long v = l;
  if (r.once) {
    if (h > 0) v = min((long long)r.l_max, v + r.l_hit);
    else if (m > 0) v = max((long long)r.l_min, v - r.l_miss);
  } else {
    if (h > 0) v = min((long long)r.l_max, v + (long long)h * r.l_hit);
    if (m > 0) v = max((long long)r.l_min, v - (long long)m * r.l_miss);
  }
  return (int)v;
}

// first index in sorted a[0, n) whose value is not below k
__device__ __forceinline__ uint32_t lower_bound_u64(const unsigned long long* __restrict__ a, uint32_t n, unsigned long long k) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Per selected point j (point j * decimation of the layer): p = (float)(R p + t) in fp64 like mh_map_insert; left out when
// non-finite, when farther than max_range from the pose's translation, when its index leaves the key range (counted);
// otherwise its end cell, M = max |e - o|, and its number of work items: M - 1 in-between cells (ray tracing) + 1 end cell.
static __global__ __launch_bounds__(256) void k_occ_rays(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ z, uint32_t n_sel, uint32_t decimation, Pose12 T,
                                                         float otx, float oty, float otz, int ox, int oy, int oz, float inv_res,
                                                         uint32_t trunc, float max_range2 /* < 0: off */, uint32_t ray_trace,
                                                         int4* __restrict__ ray_e, uint32_t* __restrict__ items,
                                                         uint32_t* __restrict__ counters /* [0]: points whose index left the range */) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_sel) return;
  const size_t i = (size_t)j * decimation;
  const double lx = x[i], ly = y[i], lz = z[i];
  const float px = (float)(((T.m[0] * lx + T.m[1] * ly) + T.m[2] * lz) + T.m[3]);
  const float py = (float)(((T.m[4] * lx + T.m[5] * ly) + T.m[6] * lz) + T.m[7]);
  const float pz = (float)(((T.m[8] * lx + T.m[9] * ly) + T.m[10] * lz) + T.m[11]);
  int4 e = make_int4(0, 0, 0, 0);
  uint32_t cnt = 0;
  if (isfinite(px) && isfinite(py) && isfinite(pz)) {
    const float dx = px - otx, dy = py - oty, dz = pz - otz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(max_range2 >= 0.f && d2 > max_range2)) {
      const float sx = px * inv_res, sy = py * inv_res, sz = pz * inv_res;
      if (fabsf(sx) < 1.0e6f && fabsf(sy) < 1.0e6f && fabsf(sz) < 1.0e6f) {
        e.x = cell_index(px, inv_res, trunc);
        e.y = cell_index(py, inv_res, trunc);
        e.z = cell_index(pz, inv_res, trunc);
        e.w = max(max(abs(e.x - ox), abs(e.y - oy)), abs(e.z - oz));
        cnt = (ray_trace && e.w > 0) ? (uint32_t)e.w : 1u;  // (M - 1) + 1
      } else {
        atomicAdd(&counters[0], 1u);
      }
    }
  }
  ray_e[j] = e;
  items[j] = cnt;
}

// The hot path.  A lane owns work item g = g0 + its index, not a ray (ray lengths differ a hundredfold): it finds its ray as
// the last one whose exclusive prefix is <= g, keeps the ray's constants in registers and writes one 8-byte key, coalesced.
// Item k_local < M - 1 is in-between cell k = k_local + 1 of the integer line walk in closed form,
//   o_a + s_a * floor((2 k ad_a + M) / (2 M))   per axis a, 64-bit integers,
// the last item of a ray is its end cell (a hit).
static __global__ __launch_bounds__(256) void k_occ_keys(const unsigned long long* __restrict__ prefix,
                                                         const int4* __restrict__ ray_e, uint32_t n_rays, int ox, int oy, int oz,
                                                         uint32_t ray_trace, unsigned long long g0, uint32_t count,
                                                         unsigned long long* __restrict__ keys) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const unsigned long long g = g0 + t;
  uint32_t lo = 0, hi = n_rays;  // first ray whose prefix is above g; the ray before it owns g
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (prefix[mid] <= g) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t r = lo - 1u;  // (prefix[0] = 0 <= g: lo >= 1)
  const int4 e = ray_e[r];
  const unsigned long long kl = g - prefix[r];
  const unsigned long long steps = (ray_trace && e.w > 0) ? (unsigned long long)(e.w - 1) : 0ull;
  unsigned long long key;
  if (kl >= steps) {
    key = pack_key(e.x, e.y, e.z) << 1;
  } else {
    const long long k = (long long)kl + 1, M = e.w;
    const int dx = e.x - ox, dy = e.y - oy, dz = e.z - oz;
    const int qx = (int)((2 * k * (long long)abs(dx) + M) / (2 * M));
    const int qy = (int)((2 * k * (long long)abs(dy) + M) / (2 * M));
    const int qz = (int)((2 * k * (long long)abs(dz) + M) / (2 * M));
    key = (pack_key(ox + (dx < 0 ? -qx : qx), oy + (dy < 0 ? -qy : qy), oz + (dz < 0 ? -qz : qz)) << 1) | 1ull;
  }
  keys[t] = key;
}

// (cell << 1 | is_miss, count) entries, sorted: head[i] = 1 on a cell's first entry (a cell has one or two, the hit first)
static __global__ __launch_bounds__(256) void k_occ_cell_heads(const unsigned long long* __restrict__ ek, uint32_t n,
                                                               uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  head[i] = (i == 0 || (ek[i - 1] >> 1) != (ek[i] >> 1)) ? 1u : 0u;
}

static __global__ __launch_bounds__(256) void k_occ_cells(const unsigned long long* __restrict__ ek, const uint32_t* __restrict__ ec,
                                                          const uint32_t* __restrict__ head, const uint32_t* __restrict__ pos,
                                                          uint32_t n, unsigned long long* __restrict__ ucell,
                                                          uint32_t* __restrict__ uh, uint32_t* __restrict__ um) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !head[i]) return;
  const unsigned long long k = ek[i], cell = k >> 1;
  uint32_t h = 0, m = 0;
  if (k & 1ull) {
    m = ec[i];
  } else {
    h = ec[i];
    if (i + 1 < n && (ek[i + 1] >> 1) == cell) m = ec[i + 1];
  }
  const uint32_t p = pos[i];
  ucell[p] = cell;
  uh[p] = h;
  um[p] = m;
}

// per touched cell: where it stands in the store, and whether it is new to it (is_new has n_u + 1 entries, the last one 0)
static __global__ __launch_bounds__(256) void k_occ_join(const unsigned long long* __restrict__ ucell, uint32_t n_u,
                                                         const unsigned long long* __restrict__ skey, uint32_t n_s,
                                                         uint32_t* __restrict__ ulb, uint32_t* __restrict__ is_new) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u > n_u) return;
  if (u == n_u) {
    is_new[u] = 0;
    return;
  }
  const unsigned long long k = ucell[u];
  const uint32_t lb = lower_bound_u64(skey, n_s, k);
  ulb[u] = lb;
  is_new[u] = (lb < n_s && skey[lb] == k) ? 0u : 1u;
}

// Threads [0, n_s): the stored cells; threads [n_s, n_s + n_u): the touched cells that are new.  Everybody computes its own
// place in the merged, ascending sequence (stored cell s: s + new cells below it; new cell u: its rank among the new ones +
// stored cells below it), applies the rule once, and leaves keep / occupied flags: keep << 32 | occupied.
static __global__ __launch_bounds__(256) void k_occ_merge(const unsigned long long* __restrict__ skey, const int* __restrict__ slo,
                                                          uint32_t n_s, const unsigned long long* __restrict__ ucell,
                                                          const uint32_t* __restrict__ uh, const uint32_t* __restrict__ um,
                                                          const uint32_t* __restrict__ ulb, const uint32_t* __restrict__ is_new,
                                                          const uint32_t* __restrict__ new_rank /* exclusive, n_u + 1 */, uint32_t n_u,
                                                          Rule rule, int4 evict /* {cx,cy,cz,dist}; w < 0: off */, uint32_t metric,
                                                          unsigned long long* __restrict__ mkey, int* __restrict__ mlo,
                                                          unsigned long long* __restrict__ flags) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_s + n_u) return;
  if (t == 0) flags[n_s + n_u] = 0ull;  // (the entry behind the last place: the scan leaves the totals there)
  unsigned long long key;
  int l;
  uint32_t pos;
  if (t < n_s) {
    key = skey[t];
    const uint32_t ub = lower_bound_u64(ucell, n_u, key);
    pos = t + new_rank[ub];
    l = slo[t];
    if (ub < n_u && ucell[ub] == key) l = apply_rule(l, uh[ub], um[ub], rule);
  } else {
    const uint32_t u = t - n_s;
    if (!is_new[u]) {
      // a touched cell the store already holds takes no place of its own: the merged sequence is n_s + (new cells) long, and
      // the places behind it, as many as there are such cells, get no flags -- each of them zeroes one, by its rank among them
      flags[n_s + new_rank[n_u] + (u - new_rank[u])] = 0ull;
      return;
    }
    key = ucell[u];
    pos = ulb[u] + new_rank[u];
    l = apply_rule(0, uh[u], um[u], rule);
  }
  int kx, ky, kz;
  unpack_key(key, kx, ky, kz);
  const bool keep = !(evict.w >= 0 && far_cell(kx - evict.x, ky - evict.y, kz - evict.z, evict.w, metric));
  mkey[pos] = key;
  mlo[pos] = l;
  flags[pos] = keep ? ((1ull << 32) | (l >= rule.l_occ ? 1ull : 0ull)) : 0ull;
}

// scan = exclusive prefix sum of the flags (n + 1 entries; the last one holds the totals)
static __global__ __launch_bounds__(256) void k_occ_compact(const unsigned long long* __restrict__ mkey, const int* __restrict__ mlo,
                                                            const unsigned long long* __restrict__ flags,
                                                            const unsigned long long* __restrict__ scan, uint32_t n, float resolution,
                                                            unsigned long long* __restrict__ okey, int* __restrict__ olo,
                                                            float* __restrict__ cx, float* __restrict__ cy, float* __restrict__ cz) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long f = flags[i];
  if (!(f >> 32)) return;
  const unsigned long long s = scan[i], key = mkey[i];
  const uint32_t p = (uint32_t)(s >> 32);
  okey[p] = key;
  olo[p] = mlo[i];
  if (f & 1ull) {
    const uint32_t q = (uint32_t)(s & 0xFFFFFFFFull);
    int kx, ky, kz;
    unpack_key(key, kx, ky, kz);
    cx[q] = ((float)kx + 0.5f) * resolution;
    cy[q] = ((float)ky + 0.5f) * resolution;
    cz[q] = ((float)kz + 0.5f) * resolution;
  }
}

}  // namespace occ
}  // namespace mh
