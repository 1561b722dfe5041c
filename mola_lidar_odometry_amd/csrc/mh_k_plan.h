// mh_k_plan.h -- kernel bodies of include/molahip_plan.h (mh_plan.hip): the cost-to-go field as sweeps of tile relaxations, the
// route trace and the field's statistics.  The rule is written down in the header.
//   k_plan_goals  one lane per goal: 0 into the field of a passable goal cell, a flag for its tile and that tile's 8 neighbours in
//                 the "changed" plane the first sweep reads, and the counters.
//   k_plan_relax  a tile of 2^lw x (1024 >> lw) cells (64 x 16 unless the window is narrower or lower, nav_tile_lw as the reach
//                 tiles) with its one-cell halo in LDS: the field as uint32 words, the price as uint16 with 0 = impassable (a cell
//                 outside the window is impassable).  A row of the image is 2^lw + 2 words: the 64 lanes of a wave read 64 consecutive
//                 words, one per bank pair, whichever neighbour they look at.  Four cells per lane; a round relaxes every cell
//                 against its 8 neighbours with plain LDS reads and writes, and rounds repeat until no lane lowered a value
//                 (__syncthreads_or).  Values only fall, and every value ever written is the length of a real path from that cell to
//                 a goal, so a value read while another lane replaces it is still an upper bound that a later round tightens; the
//                 round that changes nothing has read the final state.  The lanes then write back the cells they lowered, raise the
//                 sweep's flag and the tile's byte in the "changed in this sweep" plane.
//                 A halo word read while the neighbouring tile writes it is harmless for the same reason: the words are aligned and
//                 32 bits wide (a load sees the old or the new value, never a mix), values fall monotonically and each is a real
//                 path's length, so the tile computes upper bounds; the neighbour's write raises its "changed" byte, which makes this
//                 tile run again in the next sweep; and the sweep that changes nothing anywhere has read the final state everywhere.
//                 ACTIVE TILES.  A tile stages only when it or one of its 8 neighbour tiles has its byte set in the "changed in the
//                 previous sweep" plane (or all_tiles is set): a tile's result is a function of its cells and its halo, those change
//                 only when the tile itself or a neighbour writes, and both raise a byte.
//   k_plan_trace  one wave per start.  Lanes 0 .. 7 price the eight neighbours of the current cell in the tie order of the header, a
//                 reduction over those lanes picks the smallest (value, direction); lane 0 writes the cell.
//   k_plan_stats  the cells with a finite field and the largest finite value: a sum and a max per wave, one integer atomic each.
// No workgroup waits for another; the only atomics are integer counters.
#pragma once
#include "mh_k_nav.h"

namespace mh {
namespace plan {

constexpr uint32_t kUnreached = 0xFFFFFFFFu;
constexpr uint32_t kPlanCells = 1024u, kPlanLds = 3080u;  // entries: (2^lw + 2) * ((1024 >> lw) + 2) <= 3078 (nav_reach_lds)
constexpr uint32_t kStepOrth = 5u, kStepDiag = 7u;

// the eight neighbours in the tie order of the trace rule: E, N, W, S, NE, NW, SW, SE
__device__ __constant__ const int kDx[8] = {1, 0, -1, 0, 1, -1, -1, 1};
__device__ __constant__ const int kDy[8] = {0, 1, 0, -1, 1, 1, -1, -1};

// ctr: {goals on impassable cells, goals on passable cells}.  changed: a byte per tile.
static __global__ __launch_bounds__(256) void k_plan_goals(const int* __restrict__ goals_xy, uint32_t n_goals, uint32_t nx, uint32_t ny,
                                                           const uint8_t* __restrict__ cost, uint32_t passable_below, uint32_t lw,
                                                           uint32_t* __restrict__ field, uint8_t* __restrict__ changed,
                                                           uint32_t* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_goals) return;
  const int x = goals_xy[2u * i], y = goals_xy[2u * i + 1u];
  if (x < 0 || y < 0 || (uint32_t)x >= nx || (uint32_t)y >= ny) return;  // (the host has counted these)
  const size_t cell = (size_t)y * nx + (size_t)x;
  if (cost[cell] >= passable_below) {
    atomicAdd(&ctr[0], 1u);
    return;
  }
  field[cell] = 0u;
  atomicAdd(&ctr[1], 1u);
  const uint32_t TH = kPlanCells >> lw, tiles_x = (nx + (1u << lw) - 1u) >> lw, tiles_y = (ny + TH - 1u) / TH;
  const int tx = (int)((uint32_t)x >> lw), ty = (int)((uint32_t)y / TH);
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      const int ux = tx + dx, uy = ty + dy;
      if (ux >= 0 && uy >= 0 && (uint32_t)ux < tiles_x && (uint32_t)uy < tiles_y) changed[(size_t)uy * tiles_x + (size_t)ux] = 1;
    }
}

// grid: ceil(nx / 2^lw) * ceil(ny / (1024 >> lw)) workgroups of 256, four cells per lane.  price: uint16 [256], 0 = impassable.
// sweep: {the sweep's flag, the tiles that staged and relaxed}.
static __global__ __launch_bounds__(256) void k_plan_relax(const uint8_t* __restrict__ cost, const uint16_t* __restrict__ price, uint32_t nx,
                                                           uint32_t ny, uint32_t lw, uint32_t all_tiles,
                                                           const uint8_t* __restrict__ changed_prev, uint8_t* __restrict__ changed_now,
                                                           uint32_t* field, uint32_t* __restrict__ sweep) {
  __shared__ uint32_t s_f[kPlanLds];
  __shared__ uint16_t s_p[kPlanLds];
  const uint32_t TW = 1u << lw, TH = kPlanCells >> lw, pitch = TW + 2u;
  const uint32_t tiles_x = (nx + TW - 1u) >> lw, tiles_y = (ny + TH - 1u) / TH;
  const uint32_t tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
  if (!all_tiles) {  // (the same bytes for every lane: a uniform branch)
    uint32_t any = 0;
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        const int ux = (int)tile_x + dx, uy = (int)tile_y + dy;
        if (ux >= 0 && uy >= 0 && (uint32_t)ux < tiles_x && (uint32_t)uy < tiles_y) any |= changed_prev[(size_t)uy * tiles_x + (size_t)ux];
      }
    if (!any) return;
  }
  const long long gx0 = (long long)(tile_x << lw) - 1, gy0 = (long long)tile_y * TH - 1;
  int seen = 0;
  for (uint32_t i = threadIdx.x; i < pitch * (TH + 2u); i += 256u) {
    const uint32_t ly = i / pitch, lx = i - ly * pitch;
    const long long gx = gx0 + lx, gy = gy0 + ly;
    uint32_t f = kUnreached;
    uint16_t p = 0;
    if (gx >= 0 && gy >= 0 && gx < (long long)nx && gy < (long long)ny) {
      const size_t cell = (size_t)gy * nx + (size_t)gx;
      p = price[cost[cell]];
      f = field[cell];
    }
    s_f[i] = f;
    s_p[i] = p;
    seen |= (f != kUnreached && p) ? 1 : 0;
  }
  if (!__syncthreads_or(seen)) return;  // no finite value in the tile or its halo: nothing can change here
  if (threadIdx.x == 0) atomicAdd(&sweep[1], 1u);
  uint32_t mine = 0;  // bit k: this lane lowered its cell k
  for (;;) {
    int changed = 0;
    for (uint32_t k = 0; k < 4u; k++) {
      const uint32_t i = threadIdx.x + k * 256u;
      const uint32_t c = ((i >> lw) + 1u) * pitch + (i & (TW - 1u)) + 1u;
      const uint32_t pc = s_p[c];
      if (!pc) continue;
      const uint32_t pe = s_p[c + 1u], pn = s_p[c + pitch], pw = s_p[c - 1u], ps = s_p[c - pitch];
      uint32_t best = s_f[c];
      // (an UNREACHED neighbour wraps round under the addition and fails `v >= f`; so would a sum beyond 32 bits)
      auto take = [&](uint32_t at, uint32_t pn_, uint32_t L) {
        const uint32_t f = s_f[at], v = f + L * (pc + pn_);
        if (v >= f && v < best) best = v;
      };
      if (pe) take(c + 1u, pe, kStepOrth);
      if (pn) take(c + pitch, pn, kStepOrth);
      if (pw) take(c - 1u, pw, kStepOrth);
      if (ps) take(c - pitch, ps, kStepOrth);
      uint32_t pd;
      if (pe && pn && (pd = s_p[c + pitch + 1u])) take(c + pitch + 1u, pd, kStepDiag);
      if (pw && pn && (pd = s_p[c + pitch - 1u])) take(c + pitch - 1u, pd, kStepDiag);
      if (pw && ps && (pd = s_p[c - pitch - 1u])) take(c - pitch - 1u, pd, kStepDiag);
      if (pe && ps && (pd = s_p[c - pitch + 1u])) take(c - pitch + 1u, pd, kStepDiag);
      if (best < s_f[c]) {
        s_f[c] = best;
        mine |= 1u << k;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  if (!mine) return;
  for (uint32_t k = 0; k < 4u; k++) {
    if (!(mine & (1u << k))) continue;
    const uint32_t i = threadIdx.x + k * 256u;
    const uint32_t gx = (tile_x << lw) + (i & (TW - 1u)), gy = tile_y * TH + (i >> lw);  // (inside the window: the cell is passable)
    field[(size_t)gy * nx + gx] = s_f[((i >> lw) + 1u) * pitch + (i & (TW - 1u)) + 1u];
  }
  changed_now[blockIdx.x] = 1;
  sweep[0] = 1u;
}

// grid: ceil(n_starts / 4) workgroups of 256: a wave per start.  out_xy: n_starts * cap pairs; out_len: n_starts.
static __global__ __launch_bounds__(256) void k_plan_trace(const uint8_t* __restrict__ cost, const uint16_t* __restrict__ price,
                                                           const uint32_t* __restrict__ field, uint32_t nx, uint32_t ny,
                                                           const int* __restrict__ starts_xy, uint32_t n_starts, uint32_t cap,
                                                           int* __restrict__ out_xy, uint32_t* __restrict__ out_len) {
  const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (s >= n_starts) return;  // (the whole wave)
  int x = starts_xy[2u * s], y = starts_xy[2u * s + 1u];
  uint32_t len = 0;
  if (x >= 0 && y >= 0 && (uint32_t)x < nx && (uint32_t)y < ny) {
    uint32_t f = field[(size_t)y * nx + (size_t)x];
    if (f != kUnreached) {
      int* const out = out_xy + (size_t)s * cap * 2u;
      for (uint32_t k = 0;; k++) {  // (at most cap + 1 rounds)
        if (k == cap) {
          len = kUnreached;  // MH_PLAN_TRUNCATED: a further cell exists
          break;
        }
        if (lane == 0) {
          out[2u * k] = x;
          out[2u * k + 1u] = y;
        }
        len = k + 1u;
        if (f == 0u) break;
        unsigned long long key = ~0ull;  // (value << 3 | direction); lanes 8 .. 63 offer nothing
        if (lane < 8u) {
          const int dx = kDx[lane], dy = kDy[lane], ux = x + dx, uy = y + dy;
          if (ux >= 0 && uy >= 0 && (uint32_t)ux < nx && (uint32_t)uy < ny) {
            const uint32_t pc = price[cost[(size_t)y * nx + (size_t)x]], pu = price[cost[(size_t)uy * nx + (size_t)ux]];
            bool ok = pu != 0u;
            if (ok && lane >= 4u) ok = price[cost[(size_t)y * nx + (size_t)ux]] != 0u && price[cost[(size_t)uy * nx + (size_t)x]] != 0u;
            const uint32_t fu = field[(size_t)uy * nx + (size_t)ux];
            if (ok && fu != kUnreached)
              key = (((unsigned long long)fu + (unsigned long long)((lane < 4u ? kStepOrth : kStepDiag) * (pc + pu))) << 3) | lane;
          }
        }
        for (int off = 4; off > 0; off >>= 1) {
          const unsigned long long o = __shfl_xor(key, off, 64);
          key = o < key ? o : key;
        }
        key = __shfl(key, 0, 64);
        if (key == ~0ull || (key >> 3) != (unsigned long long)f) break;  // (cannot be on a valid field: the route ends here)
        const uint32_t d = (uint32_t)(key & 7ull);
        x += kDx[d];
        y += kDy[d];
        f = field[(size_t)y * nx + (size_t)x];
      }
    }
  }
  if (lane == 0) out_len[s] = len;
}

// stats: {cells with a finite value, the largest finite value}
static __global__ __launch_bounds__(256) void k_plan_stats(const uint32_t* __restrict__ field, size_t n, uint32_t* __restrict__ stats) {
  uint32_t sum = 0, top = 0;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
    const uint32_t f = field[i];
    if (f != kUnreached) {
      sum++;
      top = max(top, f);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_xor(sum, off, 64);
    top = max(top, (uint32_t)__shfl_xor(top, off, 64));
  }
  if ((threadIdx.x & 63u) == 0u && sum) {
    atomicAdd(&stats[0], sum);
    atomicMax(&stats[1], top);
  }
}

}  // namespace plan
}  // namespace mh
