// mh_k_elev.h -- kernel bodies of include/molahip_elevation.h (mh_elev.hip): the three point passes over a group of posed
// key-frames and the relief stencil over the ground plane.  The rule is written down in the header.
//   k_elev_points<MODE>  one lane per point of the pass, 256-lane workgroups.  The lane's frame is found as k_compose_frames
//                        finds it (frame_of, FrameSrc and the composition are mh_k_frame_src.h's): wave-uniform upper-bound
//                        searches for the wave's first and last point; where they agree pose and array pointers are read through uniform addresses.
//                        MODE 0 (bounds): the wave reduces min / max of (ix, iy); one lane issues an integer atomic for each of
//                                         the four that improves on what the bound already reads (a stale read only reads a
//                                         looser bound: a few hundred atomics on one address cost more than the pass's loads).
//                        MODE 1 (add):    atomicMin on ground, atomicAdd on count, neither returning a value, one pair per RUN of
//                                         neighbouring lanes that fall into the same cell (a segmented scan over the wave).
//                        MODE 2 (mark):   a plain load of the frozen ground, atomicMax on top, atomicAdd on obstacle_count.
//                        The two left-out counters are reduced per wave with ballot + popcount into one 64-bit atomic per wave
//                        and counter, issued only when the wave has something to add, into one of 64 slots (a cache line each,
//                        chosen by the workgroup): with a range limit most waves of a pass have something to add.
//   k_elev_relief        a 32 x 8 tile of cells per workgroup; the tile and its halo of `radius` (<= 4) cells are staged in LDS as
//                        a min plane and a max plane (unknown cells and cells outside the grid carry the neutral INT32_MAX /
//                        INT32_MIN), reduced along rows into a second pair of planes, then along columns in registers.
// Integer atomics only; nothing waits on another thread.
#pragma once
#include "mh_internal.h"
#include "mh_k_frame_src.h"

namespace mh {
namespace elev {

constexpr int kTileX = 32, kTileY = 8, kMaxR = 4;
constexpr int kHaloW = kTileX + 2 * kMaxR, kHaloH = kTileY + 2 * kMaxR;

struct Window {
  int x0, y0;
  uint32_t nx, ny;
};

enum { kBounds = 0, kAdd = 1, kMark = 2 };

// what a pass leaves besides the planes: the bounds (min x, min y, max x, max y) and, per slot, the points of cases 1 to 3 and of
// case 4; the host sums the slots
constexpr uint32_t kCounterSlots = 64;
struct Counters {
  int lo[2], hi[2];
  unsigned long long pad_[6];
  struct Slot {
    unsigned long long left_out, outside, pad_[6];
  } slot[kCounterSlots];
};
static_assert(sizeof(Counters) == 64 + 64 * kCounterSlots, "one cache line per slot");

__device__ __forceinline__ void wave_count(unsigned long long* __restrict__ dst, bool flag) {
  const unsigned long long m = __ballot(flag);
  if (m != 0ull && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(dst, (unsigned long long)__popcll(m));
}

// steps 0 to 3 of the point rule for point j of frame entry s; true when the point passes.  use_z: the height part of case 3.
template <class FramePtr>
__device__ __forceinline__ bool elev_point(FramePtr s, uint32_t j, float inv, float invq, float max_range2, bool use_z, int& ix,
                                           int& iy, int& zq) {
  float px, py, pz;
  compose_posed_point(s, j, px, py, pz);
  if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return false;
  if (max_range2 >= 0.f) {
    const float dx = px - (float)s->T[3], dy = py - (float)s->T[7], dz = pz - (float)s->T[11];
    if ((dx * dx + dy * dy) + dz * dz > max_range2) return false;
  }
  const float sx = px * inv, sy = py * inv, sz = pz * invq;
  if (!(fabsf(sx) < 1.0e6f && fabsf(sy) < 1.0e6f)) return false;
  if (use_z && !(fabsf(sz) < 1073741824.0f)) return false;
  ix = (int)floorf(sx);
  iy = (int)floorf(sy);
  zq = use_z ? (int)floorf(sz) : 0;
  return true;
}

template <int MODE>
static __global__ __launch_bounds__(256) void k_elev_points(const uint32_t* __restrict__ start, const FrameSrc* __restrict__ fr,
                                                            uint32_t n_frames, uint32_t total, float inv, float invq,
                                                            float max_range2 /* < 0: off */, Window w, int clearance_q, int step_q,
                                                            int* __restrict__ ground, uint32_t* __restrict__ count,
                                                            uint32_t* __restrict__ obstacle, int* __restrict__ top,
                                                            Counters* __restrict__ ctr) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  const uint32_t q_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(q & ~63u));  // (wave-uniform)
  if (q_first >= total) return;
  const uint32_t q_last = min(q_first + 63u, total - 1u);
  const uint32_t f_first = frame_of(start, 0u, n_frames - 1u, q_first);
  const uint32_t f_last = frame_of(start, f_first, n_frames - 1u, q_last);
  const bool live = q < total;  // (the lanes behind the last point stay for the wave's reductions)
  int ix = 0, iy = 0, zq = 0;
  bool pass = false;
  if (live) {
    if (f_first == f_last) {  // (wave-uniform branch)
      pass = elev_point((const FrameSrc __attribute__((address_space(4)))*)(fr + f_first), q - start[f_first], inv, invq, max_range2,
                        MODE != kBounds, ix, iy, zq);
    } else {
      const uint32_t f = frame_of(start, f_first, f_last, q);
      pass = elev_point((const FrameSrc __attribute__((address_space(1)))*)(fr + f), q - start[f], inv, invq, max_range2,
                        MODE != kBounds, ix, iy, zq);
    }
  }
  Counters::Slot* __restrict__ slot = &ctr->slot[blockIdx.x & (kCounterSlots - 1u)];
  wave_count(&slot->left_out, live && !pass);
  if (MODE == kBounds) {
    int lx = pass ? ix : 0x7FFFFFFF, ly = pass ? iy : 0x7FFFFFFF, hx = pass ? ix : (int)0x80000000, hy = pass ? iy : (int)0x80000000;
    for (int off = 32; off > 0; off >>= 1) {
      lx = min(lx, __shfl_xor(lx, off, 64));
      ly = min(ly, __shfl_xor(ly, off, 64));
      hx = max(hx, __shfl_xor(hx, off, 64));
      hy = max(hy, __shfl_xor(hy, off, 64));
    }
    if ((threadIdx.x & 63u) == 0u && lx <= hx) {  // (a wave without a passing point has nothing to say)
      if (lx < __hip_atomic_load(&ctr->lo[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&ctr->lo[0], lx);
      if (ly < __hip_atomic_load(&ctr->lo[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&ctr->lo[1], ly);
      if (hx > __hip_atomic_load(&ctr->hi[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&ctr->hi[0], hx);
      if (hy > __hip_atomic_load(&ctr->hi[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&ctr->hi[1], hy);
    }
    return;
  }
  const long long cx = (long long)ix - w.x0, cy = (long long)iy - w.y0;
  const bool inside = pass && cx >= 0 && cy >= 0 && cx < (long long)w.nx && cy < (long long)w.ny;
  wave_count(&slot->outside, pass && !inside);
  if (MODE == kAdd) {
    // A spinning lidar delivers a ring point after point, so near the vehicle runs of neighbouring lanes fall into one cell: a run
    // hands its minimum and its count to its last lane (a segmented scan over the wave), which issues the two atomics.  Measured
    // (profiles/traversability.md): 4.2 times the points per second of one pair of atomics per point, the same bits.
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t key = inside ? (uint32_t)((size_t)cy * w.nx + (size_t)cx) : 0xFFFFFFFFu - lane;
    int mn = zq;
    uint32_t cnt = 1u;
    const uint32_t below = __shfl_up(key, 1, 64), above = __shfl_down(key, 1, 64);  // (every lane shuffles: a lane that sits out hands out nothing)
    int f = (lane == 0u || below != key) ? 1 : 0;
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
      const int omn = __shfl_up(mn, d, 64), of = __shfl_up(f, d, 64);
      const uint32_t oc = __shfl_up(cnt, d, 64);
      if (lane >= d && !f) {
        mn = min(mn, omn);
        cnt += oc;
        f = of;
      }
    }
    const bool tail = lane == 63u || above != key;
    if (inside && tail) {
      (void)__hip_atomic_fetch_min(&ground[key], mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_add(&count[key], cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  if (!inside) return;
  const size_t c = (size_t)cy * w.nx + (size_t)cx;  // (< nx * ny <= 2^26)
  const long long h = (long long)zq - (long long)ground[c];  // (pass 2)
  if (h > (long long)clearance_q) return;  // overhead
  (void)__hip_atomic_fetch_max(&top[c], zq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (h > (long long)step_q) (void)__hip_atomic_fetch_add(&obstacle[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the planes as after mh_elev_create
static __global__ __launch_bounds__(256) void k_elev_fill(int* __restrict__ ground, uint32_t* __restrict__ count,
                                                          uint32_t* __restrict__ obstacle, int* __restrict__ top, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  ground[i] = 0x7FFFFFFF;
  count[i] = 0u;
  obstacle[i] = 0u;
  top[i] = (int)0x80000000;
}

// grid: ceil(nx / 32) * ceil(ny / 8) workgroups, one per tile, rows of tiles behind one another (a window of 2^26 cells in one
// column has more rows of tiles than a grid has in y); block: 256 = 32 x 8.  radius <= kMaxR (the host refuses more).
static __global__ __launch_bounds__(256) void k_elev_relief(const int* __restrict__ ground, const uint32_t* __restrict__ count,
                                                            uint32_t nx, uint32_t ny, int radius, uint32_t min_points,
                                                            int* __restrict__ relief) {
  __shared__ int s_min[kHaloH][kHaloW + 1], s_max[kHaloH][kHaloW + 1];  // the tile with its halo
  __shared__ int r_min[kHaloH][kTileX + 1], r_max[kHaloH][kTileX + 1];  // ... reduced along rows
  const int tx = threadIdx.x & (kTileX - 1), ty = threadIdx.x / kTileX;
  const uint32_t tiles_x = (nx + kTileX - 1u) / kTileX, tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
  const long long gx0 = (long long)tile_x * kTileX - radius, gy0 = (long long)tile_y * kTileY - radius;
  const int W = kTileX + 2 * radius, H = kTileY + 2 * radius;
  for (int i = threadIdx.x; i < W * H; i += 256) {
    const int lx = i % W, ly = i / W;
    const long long gx = gx0 + lx, gy = gy0 + ly;
    int lo = 0x7FFFFFFF, hi = (int)0x80000000;
    if (gx >= 0 && gy >= 0 && gx < (long long)nx && gy < (long long)ny) {
      const size_t c = (size_t)gy * nx + (size_t)gx;
      if (count[c] >= min_points) lo = hi = ground[c];
    }
    s_min[ly][lx] = lo;
    s_max[ly][lx] = hi;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTileX * H; i += 256) {
    const int lx = i % kTileX, ly = i / kTileX;
    int lo = 0x7FFFFFFF, hi = (int)0x80000000;
    for (int d = 0; d <= 2 * radius; d++) {
      lo = min(lo, s_min[ly][lx + d]);
      hi = max(hi, s_max[ly][lx + d]);
    }
    r_min[ly][lx] = lo;
    r_max[ly][lx] = hi;
  }
  __syncthreads();
  const uint32_t gx = tile_x * kTileX + tx, gy = tile_y * kTileY + ty;
  if (gx >= nx || gy >= ny) return;
  int lo = 0x7FFFFFFF, hi = (int)0x80000000;
  for (int d = 0; d <= 2 * radius; d++) {
    lo = min(lo, r_min[ty + d][tx]);
    hi = max(hi, r_max[ty + d][tx]);
  }
  // (a known cell is in its own window, so lo <= hi; heights lie inside (-2^30, 2^30): the difference fits)
  const bool known = s_min[ty + radius][tx + radius] <= s_max[ty + radius][tx + radius];
  relief[(size_t)gy * nx + gx] = known ? hi - lo : (int)0x80000000;
}

}  // namespace elev
}  // namespace mh
