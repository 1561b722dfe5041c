// mh_k_place.h -- place recognition by a polar height descriptor (included by mh_place.hip; the specification of descriptor
// and search is in include/molahip.h at mh_place_describe / mh_place_search).  Three kernels:
//   k_place_describe: one lane per point of a whole pass of frames, coalesced SoA reads.  A workgroup owns kPlaceChunk consecutive
//                     points of the pass; the frames they belong to are found by wave-uniform upper-bound searches in the
//                     prefix array (k_compose_frames' search) and visited one after the other -- ten thousand points per
//                     frame: one frame per workgroup, rarely two.  Per frame the workgroup keeps R*S 32-bit bins in LDS (at most
//                     16 KB), zeroed; points go in with atomicMax in LDS; only the non-zero bins are flushed, with a global
//                     integer atomicMax into the frame's zeroed 32-bit bins.  Integer maxima: exact whatever the arrival order.
//   k_place_pack:     the 32-bit bins narrowed to the descriptor's bytes.
//   k_place_search:   the query against every stored descriptor under all S column shifts.  The query sits in LDS with its
//                     columns doubled, so a shift is an offset and not a modulo; a group of S*G lanes (G ring groups) serves one
//                     stored descriptor, which it stages once; lane = (shift, ring group).  Four bins per instruction:
//                     v_alignbyte_b32 builds the byte-shifted dword of the query, v_sad_u8 accumulates.  The ring groups' sums
//                     meet in LDS (integer adds), the packed key dist << 7 | shift is reduced to its minimum there.
// The tables are kernel arguments (wave-uniform: scalar loads).  All point arithmetic is un-fused fp32 (-ffp-contract=off).
#pragma once
#include <stdint.h>

#include "mh_place_bin.h"

namespace mh {

constexpr uint32_t kPlaceMaxBins = MH_PLACE_MAX_RINGS * MH_PLACE_MAX_SECTORS;

struct PlaceTables {  // built on the host in fp64, rounded once (place_make_tables, mh_place.hip)
  float ring_edge2[MH_PLACE_MAX_RINGS + 1];
  float tan_edge[MH_PLACE_MAX_SECTORS / 8];  // [0] unused: j = 1 .. S/8-1
  float z_min, z_max, zscale;
  uint32_t R, S;
};

// bin (ring * S + sector) and level (1..255) of one point; false: the point is skipped
__device__ __forceinline__ bool place_bin(const PlaceTables& t, float x, float y, float z, uint32_t& bin, uint32_t& level) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  if (x == 0.f && y == 0.f) return false;
  const float r2 = x * x + y * y;
  if (!(r2 >= t.ring_edge2[0] && r2 < t.ring_edge2[t.R])) return false;
  if (!(z >= t.z_min && z < t.z_max)) return false;
  uint32_t ring = 0;
  for (uint32_t k = 1; k < t.R; k++) ring += t.ring_edge2[k] <= r2 ? 1u : 0u;
  level = min(255u, 1u + (uint32_t)((z - t.z_min) * t.zscale));
  bin = ring * t.S + place_sector(t.tan_edge, t.S, x, y);
  return true;
}

// bins32[f * R*S + bin] = max(.., level) over the points of frame f; the caller has zeroed bins32 [n_frames * R*S]
__global__ __launch_bounds__(kPlaceBlock) void k_place_describe(const uint32_t* __restrict__ start, const PlaceSrc* __restrict__ fr,
                                                                uint32_t n_frames, uint32_t total, PlaceTables tab,
                                                                uint32_t* __restrict__ bins32) {
  __shared__ uint32_t sh_bins[kPlaceMaxBins];
  const uint32_t q0 = blockIdx.x * kPlaceChunk;  // (uniform; the grid covers `total`: q0 < total)
  const uint32_t q1 = min(q0 + kPlaceChunk, total);
  const uint32_t RS = tab.R * tab.S;
  const uint32_t f_first = place_frame_of(start, 0u, n_frames - 1u, q0);
  const uint32_t f_last = place_frame_of(start, f_first, n_frames - 1u, q1 - 1u);
  for (uint32_t f = f_first; f <= f_last; f++) {  // (uniform trip count)
    const uint32_t lo = max(start[f], q0), hi = min(start[f + 1u], q1);
    if (lo >= hi) continue;  // (an empty frame between two others; uniform)
    for (uint32_t i = threadIdx.x; i < RS; i += kPlaceBlock) sh_bins[i] = 0u;
    __syncthreads();
    const float* __restrict__ fx = fr[f].x;
    const float* __restrict__ fy = fr[f].y;
    const float* __restrict__ fz = fr[f].z;
    const uint32_t base = start[f];
    for (uint32_t q = lo + threadIdx.x; q < hi; q += kPlaceBlock) {
      const uint32_t j = q - base;
      uint32_t bin, level;
      if (place_bin(tab, fx[j], fy[j], fz[j], bin, level)) atomicMax(&sh_bins[bin], level);
    }
    __syncthreads();
    uint32_t* __restrict__ out = bins32 + (size_t)f * RS;
    for (uint32_t i = threadIdx.x; i < RS; i += kPlaceBlock) {
      const uint32_t v = sh_bins[i];
      if (v) atomicMax(&out[i], v);
    }
    __syncthreads();  // (the bins are zeroed again for the next frame)
  }
}

__global__ __launch_bounds__(256) void k_place_pack(const uint32_t* __restrict__ bins32, size_t n, uint8_t* __restrict__ desc) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) desc[i] = (uint8_t)bins32[i];
}

// Geometry of the search, the same on host and device: G ring groups (a power of two, at most R and at most 256 / S), a group
// of L = S * G lanes per stored descriptor, n_sub = 256 / L descriptors per workgroup and round.
struct PlaceSearchGeom {
  uint32_t G, L, n_sub;
};
__host__ __device__ inline PlaceSearchGeom place_search_geom(uint32_t R, uint32_t S) {
  PlaceSearchGeom g;
  g.G = 1;
  while (g.G * 2u <= R && g.G * 2u * S <= kPlaceBlock) g.G *= 2u;
  g.L = S * g.G;
  g.n_sub = kPlaceBlock / g.L;
  return g;
}

// LDS of k_place_search, in dwords: the doubled query R * S/2, one stored descriptor per sub-group (R*S/4 each; n_sub * R*S/4
// <= 1024), the per-shift sums n_sub * S <= 256, the keys n_sub <= 32
constexpr uint32_t kPlaceQueryDwords = MH_PLACE_MAX_RINGS * (MH_PLACE_MAX_SECTORS / 2);
constexpr uint32_t kPlaceStoredDwords = kPlaceMaxBins / 4;

__global__ __launch_bounds__(kPlaceBlock) void k_place_search(const uint32_t* __restrict__ stored, uint32_t K,
                                                              const uint32_t* __restrict__ query, uint32_t R, uint32_t S,
                                                              mh_place_match* __restrict__ out) {
  __shared__ uint32_t sh_q[kPlaceQueryDwords];  // row r: S/2 dwords = the ring's S bytes twice
  __shared__ uint32_t sh_d[kPlaceStoredDwords];
  __shared__ uint32_t sh_sum[kPlaceBlock];
  __shared__ uint32_t sh_key[32];
  const PlaceSearchGeom g = place_search_geom(R, S);
  const uint32_t S4 = S >> 2, RS4 = R * S4;  // dwords per ring / per descriptor
  for (uint32_t i = threadIdx.x; i < 2u * RS4; i += kPlaceBlock) {
    const uint32_t r = i / (2u * S4), c = i - r * 2u * S4;
    sh_q[i] = query[r * S4 + (c >= S4 ? c - S4 : c)];
  }
  const uint32_t sub = threadIdx.x / g.L, t = threadIdx.x - sub * g.L;  // lanes beyond n_sub * L idle (sub == n_sub)
  const uint32_t grp = t / S, s = t - grp * S;                           // ring group, shift
  const uint32_t sd = s >> 2, sb = s & 3u;
  const uint32_t n_rounds = (K + g.n_sub - 1u) / g.n_sub;
  for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {  // (uniform)
    const uint32_t k = round * g.n_sub + sub;
    const bool active = sub < g.n_sub && k < K;
    __syncthreads();  // the query is staged / the previous round's LDS is read
    if (active) {
      const uint32_t* __restrict__ src = stored + (size_t)k * RS4;
      for (uint32_t i = t; i < RS4; i += g.L) sh_d[sub * RS4 + i] = src[i];
      if (grp == 0) sh_sum[sub * S + s] = 0u;
      if (t == 0) sh_key[sub] = 0xFFFFFFFFu;
    }
    __syncthreads();
    if (active) {
      uint32_t acc = 0;
      for (uint32_t r = grp; r < R; r += g.G) {
        const uint32_t* qrow = sh_q + r * 2u * S4 + sd;
        const uint32_t* drow = sh_d + sub * RS4 + r * S4;
        uint32_t lo = qrow[0];
        for (uint32_t c = 0; c < S4; c++) {
          const uint32_t hi = qrow[c + 1u];  // (c + 1 + sd <= S4 + S4 - 1: inside the doubled row)
          acc = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, sb), drow[c], acc);
          lo = hi;
        }
      }
      atomicAdd(&sh_sum[sub * S + s], acc);
    }
    __syncthreads();
    if (active && grp == 0) atomicMin(&sh_key[sub], (sh_sum[sub * S + s] << 7) | s);
    __syncthreads();
    if (active && t == 0) {
      const uint32_t key = sh_key[sub];
      mh_place_match m;
      m.shift = key & 127u;
      m.dist = key >> 7;
      out[k] = m;
    }
  }
}

}  // namespace mh
