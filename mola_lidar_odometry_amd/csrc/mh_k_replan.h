// mh_k_replan.h -- kernel bodies of include/molahip_replan.h (mh_replan.hip): the patch of a rectangle of the cost plane and the
// withdrawal of the field values that rested on what the patch took away.  The rule is written down in the header.
//   k_replan_patch     one lane per rectangle cell: compares the old byte with the new one, writes the new one and counts the cells
//                      whose byte differs and those whose price differs (price[] holds 0 for an impassable byte, so one comparison
//                      covers passability and price).  A cell that is now impassable gets MH_PLAN_UNREACHED (counted when its value was
//                      finite: it is withdrawn by definition).  For a repriced cell it raises the byte of its tile AND OF THAT TILE'S 8
//                      NEIGHBOURS in the "changed" plane the first withdraw sweep reads and in the accumulating "touched" plane the
//                      relax sweeps start from: the cell may be a halo cell of those tiles, or one of the two cells a diagonal step
//                      between cells of two other tiles passes, so their cells' support -- or their relaxation -- may have changed
//                      though none of their own bytes did.  Without a valid field (`field` NULL) it replaces and counts bytes only.
//   k_replan_withdraw  k_plan_relax's tile and LDS image unchanged: 2^lw x (1024 >> lw) cells with a one-cell halo, the field as uint32
//                      words, the price as uint16 with 0 = impassable, four cells per lane.  A round takes back (sets to UNREACHED)
//                      every finite cell with value > 0 that has no supporting neighbour: no passable n, by a step the field rule
//                      allows, with a finite F[n] and F[n] + w(c, n) <= F[c].  Rounds repeat until no lane takes a value back
//                      (__syncthreads_or).  The lanes then write back what they withdrew, count it, and raise the tile's byte in the
//                      "changed in this sweep" plane, the sweep's flag and the tile's byte in the "touched" plane.
//                      THE RACES.  Values only go from finite to UNREACHED, and only the lane that owns a cell writes it.  Inside a
//                      round a lane may read a neighbour's word while its owner replaces it: the words are aligned and 32 bits wide,
//                      so it sees the old value or UNREACHED.  The old value shows a supporter that is about to go, which only delays
//                      the withdrawal to the next round; the round in which nobody writes has read the final state of the tile.  A halo
//                      word read while the neighbouring tile withdraws it is stale in the same harmless direction: a cell is never
//                      withdrawn because of it, only kept for now; the neighbour's write raises its "changed" byte, so this tile runs
//                      again in the next sweep; and the sweep that changes nothing anywhere has read the final state everywhere.  What
//                      is left then supports itself, so it lies in the largest self-supporting set K of the header; and no cell of K is
//                      ever taken back, because its supporter in K is still there whenever it is looked at.  What is left is K.
//                      ACTIVE TILES as k_plan_relax: a tile stages only when it or one of its 8 neighbour tiles has its byte set in the
//                      "changed in the previous sweep" plane (or all_tiles is set).
// No workgroup waits for another; the only atomics are integer counters.  Every store is a plain vector store.
#pragma once
#include "mh_k_plan.h"

namespace mh {
namespace plan {

// grid: ceil(w * h / 256) workgroups of 256.  src: the new bytes, row r of the rectangle at src + r * src_pitch.
// ctr: {cells changed, cells repriced, cells closed that had a finite field}.  changed, touched: a byte per tile.
static __global__ __launch_bounds__(256) void k_replan_patch(const uint8_t* __restrict__ src, size_t src_pitch, uint32_t x0, uint32_t y0,
                                                             uint32_t w, uint32_t h, uint32_t nx, uint32_t ny, uint32_t lw,
                                                             const uint16_t* __restrict__ price, uint8_t* __restrict__ cost,
                                                             uint32_t* field, uint8_t* __restrict__ changed, uint8_t* __restrict__ touched,
                                                             uint32_t* __restrict__ ctr) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  bool differs = false, repriced = false, closed = false;
  if (i < (size_t)w * h) {
    const uint32_t r = (uint32_t)(i / w), c = (uint32_t)(i - (size_t)r * w);
    const uint32_t x = x0 + c, y = y0 + r;  // (inside the window: the host has checked the rectangle)
    const size_t cell = (size_t)y * nx + x;
    const uint8_t was = cost[cell], now = src[(size_t)r * src_pitch + c];
    if (was != now) {
      differs = true;
      cost[cell] = now;
      if (field) {
        const uint16_t p_now = price[now];
        repriced = price[was] != p_now;
        if (repriced) {
          if (!p_now) {
            closed = field[cell] != kUnreached;
            field[cell] = kUnreached;
          }
          const uint32_t TH = kPlanCells >> lw, tiles_x = (nx + (1u << lw) - 1u) >> lw, tiles_y = (ny + TH - 1u) / TH;
          const int tx = (int)(x >> lw), ty = (int)(y / TH);
          for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
              const int ux = tx + dx, uy = ty + dy;
              if (ux >= 0 && uy >= 0 && (uint32_t)ux < tiles_x && (uint32_t)uy < tiles_y) {
                changed[(size_t)uy * tiles_x + (size_t)ux] = 1;
                touched[(size_t)uy * tiles_x + (size_t)ux] = 1;
              }
            }
        }
      }
    }
  }
  const uint32_t n_d = (uint32_t)__popcll(__ballot(differs)), n_r = (uint32_t)__popcll(__ballot(repriced)),
                 n_c = (uint32_t)__popcll(__ballot(closed));
  if ((threadIdx.x & 63u) == 0u) {
    if (n_d) atomicAdd(&ctr[0], n_d);
    if (n_r) atomicAdd(&ctr[1], n_r);
    if (n_c) atomicAdd(&ctr[2], n_c);
  }
}

// grid: ceil(nx / 2^lw) * ceil(ny / (1024 >> lw)) workgroups of 256, four cells per lane.  price: uint16 [256], 0 = impassable.
// sweep: {the sweep's flag, the tiles that staged, the cells withdrawn}.
static __global__ __launch_bounds__(256) void k_replan_withdraw(const uint8_t* __restrict__ cost, const uint16_t* __restrict__ price,
                                                                uint32_t nx, uint32_t ny, uint32_t lw, uint32_t all_tiles,
                                                                const uint8_t* __restrict__ changed_prev, uint8_t* __restrict__ changed_now,
                                                                uint8_t* __restrict__ touched, uint32_t* field, uint32_t* __restrict__ sweep) {
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
    // a value above 0 inside the tile proper: only such a cell can be taken back here
    seen |= (f != kUnreached && f && p && lx >= 1u && lx <= TW && ly >= 1u && ly <= TH) ? 1 : 0;
  }
  if (!__syncthreads_or(seen)) return;
  if (threadIdx.x == 0) atomicAdd(&sweep[1], 1u);
  uint32_t mine = 0;  // bit k: this lane took its cell k back
  for (;;) {
    int changed = 0;
    for (uint32_t k = 0; k < 4u; k++) {
      const uint32_t i = threadIdx.x + k * 256u;
      const uint32_t c = ((i >> lw) + 1u) * pitch + (i & (TW - 1u)) + 1u;
      const uint32_t pc = s_p[c], fc = s_f[c];
      if (!pc || fc == kUnreached || !fc) continue;
      const uint32_t pe = s_p[c + 1u], pn = s_p[c + pitch], pw = s_p[c - 1u], ps = s_p[c - pitch];
      bool held = false;
      // (an UNREACHED neighbour wraps round under the addition and fails `v >= f`; so would a sum beyond 32 bits)
      auto rest = [&](uint32_t at, uint32_t pn_, uint32_t L) {
        const uint32_t f = s_f[at], v = f + L * (pc + pn_);
        if (v >= f && v <= fc) held = true;
      };
      if (pe) rest(c + 1u, pe, kStepOrth);
      if (pn) rest(c + pitch, pn, kStepOrth);
      if (pw) rest(c - 1u, pw, kStepOrth);
      if (ps) rest(c - pitch, ps, kStepOrth);
      uint32_t pd;
      if (pe && pn && (pd = s_p[c + pitch + 1u])) rest(c + pitch + 1u, pd, kStepDiag);
      if (pw && pn && (pd = s_p[c + pitch - 1u])) rest(c + pitch - 1u, pd, kStepDiag);
      if (pw && ps && (pd = s_p[c - pitch - 1u])) rest(c - pitch - 1u, pd, kStepDiag);
      if (pe && ps && (pd = s_p[c - pitch + 1u])) rest(c - pitch + 1u, pd, kStepDiag);
      if (!held) {
        s_f[c] = kUnreached;
        mine |= 1u << k;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  uint32_t n = (uint32_t)__popc(mine);
  for (uint32_t k = 0; k < 4u; k++) {
    if (!(mine & (1u << k))) continue;
    const uint32_t i = threadIdx.x + k * 256u;
    const uint32_t gx = (tile_x << lw) + (i & (TW - 1u)), gy = tile_y * TH + (i >> lw);  // (inside the window: the cell is passable)
    field[(size_t)gy * nx + gx] = kUnreached;
  }
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
  if (!n) return;  // (the whole wave)
  if ((threadIdx.x & 63u) == 0u) {
    atomicAdd(&sweep[2], n);
    changed_now[blockIdx.x] = 1;
    touched[blockIdx.x] = 1;
    sweep[0] = 1u;
  }
}

}  // namespace plan
}  // namespace mh
