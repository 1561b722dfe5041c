// mh_k_occgrid.h -- kernel bodies of include/molahip_occgrid.h (mh_occgrid.hip): the ray-traced insertion of a whole group of
// key-frames into the occupancy map, the index bounds of the stored cells and their projection to a 2-D grid.
//
// The batched insertion restates K calls of mh_occmap_insert.  The update rule clamps per insert, so frames do not commute on
// a cell: the counts stay per (cell, frame) and are folded per cell in frame order.
//   k_occf_rays        per selected point of the pass: its frame (upper bound over the pass's prefix array), then exactly
//                      k_occ_rays' arithmetic with that frame's pose and origin cell
//   (prefix sum over the items)
//   k_occf_keys        per WORK ITEM: k_occ_keys' 64-bit key  cell << 1 | is_miss  and the frame's index in the pass as a value
//   (ONE stable pair sort by key: items are generated frame after frame, so equal keys keep frame order)
//   k_occf_pair_heads, k_occf_pair_runs, k_occf_entries     run lengths over (key, frame): entries (key, frame << 32 | count)
//   (chunks of a pass: entries appended -- for one key still in frame order, the work items being generated frame after frame --,
//   sorted by key once more, stably; k_occf_sum_runs sums the entries of equal (key, frame))
//   k_occ_cell_heads (mh_k_occ.h), k_occf_cells             one slice of entries per touched cell
//   k_occf_fold        per touched cell: join with the store, walk the hit run and the miss run with two cursors in frame order
//   k_occf_merge       k_occ_merge with the folded value in place of one application of the rule
//   (prefix sum over the flags, k_occ_compact: mh_k_occ.h)
// Nothing waits on another thread, there are no float atomics; the only atomics are integer min / max / add.
#pragma once
#include "mh_k_frame_src.h"  // frame_of, compose_posed_point
#include "mh_k_occ.h"

namespace mh {
namespace occ {

// one frame of a pass (device memory, mirrored on the host byte for byte)
struct OccFrame {
  const float *x, *y, *z;  // the frame's points (device memory; never read for an empty frame)
  double T[12];            // row-major 3x4
  float ot[3];             // (float) of T's translation: the range test's origin
  int oc[3];               // the cell of T's translation: the ray origin
};
static_assert(sizeof(OccFrame) == 144, "OccFrame is mirrored on the host byte for byte");

// `start` is the prefix array of the pass's SELECTED points (every decimation-th of each frame), n_frames + 1 entries.  A wave
// whose first and last point share a frame (all but one wave per frame) finds it with wave-uniform searches and reads pose and
// pointers through uniform addresses (scalar loads); a wave that straddles frames searches per lane between those bounds.
static __global__ __launch_bounds__(256) void k_occf_rays(const uint32_t* __restrict__ start, const OccFrame* __restrict__ fr,
                                                          uint32_t n_frames, uint32_t total, uint32_t decimation, float inv_res,
                                                          uint32_t trunc, float max_range2 /* < 0: off */, uint32_t ray_trace,
                                                          int4* __restrict__ ray_e, uint32_t* __restrict__ items,
                                                          uint32_t* __restrict__ ray_f,
                                                          uint32_t* __restrict__ counters /* [0]: points whose index left the range */) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  const uint32_t q_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(q & ~63u));  // (wave-uniform)
  if (q_first >= total) return;
  const uint32_t q_last = min(q_first + 63u, total - 1u);
  const uint32_t f_first = frame_of(start, 0u, n_frames - 1u, q_first);
  const uint32_t f_last = frame_of(start, f_first, n_frames - 1u, q_last);
  if (q >= total) return;
  const uint32_t f = f_first == f_last ? f_first : frame_of(start, f_first, f_last, q);
  const OccFrame* __restrict__ s = fr + f;
  const size_t i = (size_t)(q - start[f]) * decimation;
  float px, py, pz;
  compose_posed_point(s, i, px, py, pz);
  int4 e = make_int4(0, 0, 0, 0);
  uint32_t cnt = 0;
  if (isfinite(px) && isfinite(py) && isfinite(pz)) {
    const float dx = px - s->ot[0], dy = py - s->ot[1], dz = pz - s->ot[2];
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(max_range2 >= 0.f && d2 > max_range2)) {
      const float sx = px * inv_res, sy = py * inv_res, sz = pz * inv_res;
      if (fabsf(sx) < 1.0e6f && fabsf(sy) < 1.0e6f && fabsf(sz) < 1.0e6f) {
        e.x = cell_index(px, inv_res, trunc);
        e.y = cell_index(py, inv_res, trunc);
        e.z = cell_index(pz, inv_res, trunc);
        e.w = max(max(abs(e.x - s->oc[0]), abs(e.y - s->oc[1])), abs(e.z - s->oc[2]));
        cnt = (ray_trace && e.w > 0) ? (uint32_t)e.w : 1u;  // (M - 1) + 1
      } else {
        atomicAdd(&counters[0], 1u);
      }
    }
  }
  ray_e[q] = e;
  items[q] = cnt;
  ray_f[q] = f;
}

// The hot path: k_occ_keys with the ray's frame.  One 8-byte key and one 4-byte value per lane, both coalesced.
static __global__ __launch_bounds__(256) void k_occf_keys(const unsigned long long* __restrict__ prefix, const int4* __restrict__ ray_e,
                                                          const uint32_t* __restrict__ ray_f, const OccFrame* __restrict__ fr,
                                                          uint32_t n_rays, uint32_t ray_trace, unsigned long long g0, uint32_t count,
                                                          unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
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
  const uint32_t f = ray_f[r];
  const unsigned long long kl = g - prefix[r];
  const unsigned long long steps = (ray_trace && e.w > 0) ? (unsigned long long)(e.w - 1) : 0ull;
  unsigned long long key;
  if (kl >= steps) {
    key = pack_key(e.x, e.y, e.z) << 1;
  } else {
    const int ox = fr[f].oc[0], oy = fr[f].oc[1], oz = fr[f].oc[2];
    const long long k = (long long)kl + 1, M = e.w;
    const int dx = e.x - ox, dy = e.y - oy, dz = e.z - oz;
    const int qx = (int)((2 * k * (long long)abs(dx) + M) / (2 * M));
    const int qy = (int)((2 * k * (long long)abs(dy) + M) / (2 * M));
    const int qz = (int)((2 * k * (long long)abs(dz) + M) / (2 * M));
    key = (pack_key(ox + (dx < 0 ? -qx : qx), oy + (dy < 0 ? -qy : qy), oz + (dz < 0 ? -qz : qz)) << 1) | 1ull;
  }
  keys[t] = key;
  vals[t] = f;
}

// sorted (key, frame) items: head[i] = 1 on the first item of a (key, frame) run
static __global__ __launch_bounds__(256) void k_occf_pair_heads(const unsigned long long* __restrict__ k, const uint32_t* __restrict__ v,
                                                                uint32_t n, uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  head[i] = (i == 0 || k[i - 1] != k[i] || v[i - 1] != v[i]) ? 1u : 0u;
}

// run p starts at item rstart[p]; rstart[number of runs] = n
static __global__ __launch_bounds__(256) void k_occf_pair_runs(const uint32_t* __restrict__ head, const uint32_t* __restrict__ pos,
                                                               uint32_t n, uint32_t* __restrict__ rstart) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (head[i]) rstart[pos[i]] = i;
  if (i == n - 1u) rstart[pos[i] + head[i]] = n;
}

// entry p = (key, frame << 32 | count) of run p
static __global__ __launch_bounds__(256) void k_occf_entries(const unsigned long long* __restrict__ k, const uint32_t* __restrict__ v,
                                                             const uint32_t* __restrict__ rstart, uint32_t n_runs,
                                                             unsigned long long* __restrict__ ek, unsigned long long* __restrict__ ev) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_runs) return;
  const uint32_t a = rstart[p], b = rstart[p + 1u];
  ek[p] = k[a];
  ev[p] = ((unsigned long long)v[a] << 32) | (unsigned long long)(b - a);
}

// the same for a chunk of several: key, frame and count apart (the chunks' entries are appended, then sorted by key once more)
static __global__ __launch_bounds__(256) void k_occf_entries_split(const unsigned long long* __restrict__ k, const uint32_t* __restrict__ v,
                                                                   const uint32_t* __restrict__ rstart, uint32_t n_runs,
                                                                   unsigned long long* __restrict__ ek, uint32_t* __restrict__ ef,
                                                                   uint32_t* __restrict__ ec) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_runs) return;
  const uint32_t a = rstart[p], b = rstart[p + 1u];
  ek[p] = k[a];
  ef[p] = v[a];
  ec[p] = b - a;
}

// entries of several chunks sorted by (key, frame): equal (key, frame) entries stand together, at most one per chunk; head and
// pos are k_occf_pair_heads' flags and their exclusive prefix sum
static __global__ __launch_bounds__(256) void k_occf_sum_runs(const unsigned long long* __restrict__ ek, const uint32_t* __restrict__ ef,
                                                              const uint32_t* __restrict__ ec, const uint32_t* __restrict__ head,
                                                              const uint32_t* __restrict__ pos, uint32_t n,
                                                              unsigned long long* __restrict__ ok, unsigned long long* __restrict__ ov) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !head[i]) return;
  unsigned long long c = ec[i];
  for (uint32_t j = i + 1u; j < n && !head[j]; j++) c += ec[j];
  ok[pos[i]] = ek[i];
  ov[pos[i]] = ((unsigned long long)ef[i] << 32) | (c & 0xFFFFFFFFull);
}

// touched cell p owns the entries ustart[p] .. ustart[p + 1] - 1 (its hit entries in frame order, then its miss entries)
static __global__ __launch_bounds__(256) void k_occf_cells(const unsigned long long* __restrict__ ek, const uint32_t* __restrict__ head,
                                                           const uint32_t* __restrict__ pos, uint32_t n,
                                                           unsigned long long* __restrict__ ucell, uint32_t* __restrict__ ustart) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (head[i]) {
    ucell[pos[i]] = ek[i] >> 1;
    ustart[pos[i]] = i;
  }
  if (i == n - 1u) ustart[pos[i] + head[i]] = n;
}

// One lane per touched cell (and one more that closes is_new, as k_occ_join): where the cell stands in the store, whether it
// is new to it, and its log-odds after every frame of the pass that touched it applied its own rule, in frame order.
static __global__ __launch_bounds__(256) void k_occf_fold(const unsigned long long* __restrict__ ucell,
                                                          const uint32_t* __restrict__ ustart, uint32_t n_u,
                                                          const unsigned long long* __restrict__ ek,
                                                          const unsigned long long* __restrict__ ev,
                                                          const unsigned long long* __restrict__ skey, const int* __restrict__ slo,
                                                          uint32_t n_s, Rule rule, uint32_t* __restrict__ ulb,
                                                          uint32_t* __restrict__ is_new, int* __restrict__ unew) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u > n_u) return;
  if (u == n_u) {
    is_new[u] = 0;
    return;
  }
  const unsigned long long cell = ucell[u];
  const uint32_t lb = lower_bound_u64(skey, n_s, cell);
  const bool stored = lb < n_s && skey[lb] == cell;
  ulb[u] = lb;
  is_new[u] = stored ? 0u : 1u;
  int l = stored ? slo[lb] : 0;
  const uint32_t a = ustart[u], b = ustart[u + 1u];
  const uint32_t hm = a + lower_bound_u64(ek + a, b - a, (cell << 1) | 1ull);  // hit entries [a, hm), miss entries [hm, b)
  uint32_t i = a, j = hm;
  while (i < hm || j < b) {
    const unsigned long long vh = i < hm ? ev[i] : ~0ull, vm = j < b ? ev[j] : ~0ull;
    const uint32_t fh = (uint32_t)(vh >> 32), fm = (uint32_t)(vm >> 32);  // (0xFFFFFFFF: the run is used up)
    const uint32_t f = min(fh, fm);
    uint32_t h = 0, m = 0;
    if (fh == f) { h = (uint32_t)vh; i++; }
    if (fm == f) { m = (uint32_t)vm; j++; }
    l = apply_rule(l, h, m, rule);
  }
  unew[u] = l;
}

// k_occ_merge with the value of every touched cell already folded (unew) and no far removal
static __global__ __launch_bounds__(256) void k_occf_merge(const unsigned long long* __restrict__ skey, const int* __restrict__ slo,
                                                           uint32_t n_s, const unsigned long long* __restrict__ ucell,
                                                           const int* __restrict__ unew, const uint32_t* __restrict__ ulb,
                                                           const uint32_t* __restrict__ is_new,
                                                           const uint32_t* __restrict__ new_rank /* exclusive, n_u + 1 */, uint32_t n_u,
                                                           int l_occ, unsigned long long* __restrict__ mkey, int* __restrict__ mlo,
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
    if (ub < n_u && ucell[ub] == key) l = unew[ub];
  } else {
    const uint32_t u = t - n_s;
    if (!is_new[u]) {  // (takes no place of its own: see k_occ_merge)
      flags[n_s + new_rank[n_u] + (u - new_rank[u])] = 0ull;
      return;
    }
    key = ucell[u];
    pos = ulb[u] + new_rank[u];
    l = unew[u];
  }
  mkey[pos] = key;
  mlo[pos] = l;
  flags[pos] = (1ull << 32) | (l >= l_occ ? 1ull : 0ull);
}

// ---- index bounds: integer min / max per axis.  A fixed grid strides over the cells (a lane folds its share in registers), the
// wave reduces, and one lane per wave issues the six integer atomics: at most 512 waves, 3 072 atomics, whatever the map's size.  out[0..2] =
// min, out[3..5] = max, initialised by the host to INT_MAX / INT_MIN.
static __global__ __launch_bounds__(256) void k_occ_bounds(const unsigned long long* __restrict__ skey, uint32_t n,
                                                           int* __restrict__ out) {
  int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int k[3];
    unpack_key(skey[i], k[0], k[1], k[2]);
    for (int a = 0; a < 3; a++) {
      lo[a] = min(lo[a], k[a]);
      hi[a] = max(hi[a], k[a]);
    }
  }
  for (int a = 0; a < 3; a++) {
    for (int off = 32; off > 0; off >>= 1) {
      lo[a] = min(lo[a], __shfl_xor(lo[a], off, 64));
      hi[a] = max(hi[a], __shfl_xor(hi[a], off, 64));
    }
  }
  if ((threadIdx.x & 63u) == 0u) {
    for (int a = 0; a < 3; a++) {
      atomicMin(&out[a], lo[a]);
      atomicMax(&out[3 + a], hi[a]);
    }
  }
}

// ---- projection: one lane per stored cell; the grid holds INT32_MIN where nothing was stored.  Integer atomicMax: exact and
// independent of the order of the lanes.
static __global__ __launch_bounds__(256) void k_occ_project(const unsigned long long* __restrict__ skey, const int* __restrict__ slo,
                                                            uint32_t n, int x0, int y0, uint32_t nx, uint32_t ny, int z_lo, int z_hi,
                                                            int* __restrict__ grid) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int kx, ky, kz;
  unpack_key(skey[i], kx, ky, kz);
  if (kz < z_lo || kz > z_hi) return;
  const long long cx = (long long)kx - x0, cy = (long long)ky - y0;
  if (cx < 0 || cy < 0 || cx >= (long long)nx || cy >= (long long)ny) return;
  atomicMax(&grid[(size_t)cy * nx + (size_t)cx], slo[i]);
}

static __global__ __launch_bounds__(256) void k_occ_grid_fill(int* __restrict__ grid, size_t n, int v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) grid[i] = v;
}

}  // namespace occ
}  // namespace mh
