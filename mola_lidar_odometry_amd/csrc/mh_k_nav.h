// mh_k_nav.h -- kernel bodies of include/molahip_nav.h (mh_nav.hip): the two passes of the exact distance transform with the
// inflated cost, and the flood fill of the reachable region.  The rule is written down in the header.  Unlike every other unit
// under csrc/ these are stencils over a plane, not lanes over points.
//   k_nav_col    a tile of 2^lw columns x (4096 >> lw) rows per workgroup (64 x 64 unless the window is narrower or lower).  The
//                obstacle flags of the tile and of its halo of Rh = min(R, ny - 1) rows above and below are staged in LDS as bytes
//                (a lane of a wave reads the byte next to its neighbour's: four lanes share a bank word, no conflict); a cell
//                walks outwards, one row up and one row down per step, to the first obstacle: g = that distance, or kNavNone.
//   k_nav_row    256 cells per workgroup: 2^lw cells of (256 >> lw) rows (one segment of 256 cells unless the window is narrower).
//                g of the segment and of its halo of Rh = min(R, nx - 1) cells on either side is staged in LDS as uint16; a cell
//                takes the minimum of g(x +- dx)^2 + dx^2 over dx = 0 .. Rh and, with EARLY, stops once dx^2 reaches the best
//                value found (every later candidate is at least dx^2).  It writes d2 and the cost.
//   k_nav_seed   one lane per seed.
//   k_nav_reach  a tile of 2^lw x (1024 >> lw) cells (64 x 16 unless the window is narrower or lower) with its one-cell halo in
//                LDS: passable flags and the reach bytes.  The tile relaxes until no lane changes a cell (__syncthreads_or), the
//                lanes write back the cells they set and store 1 to the sweep's flag.  Cells only ever go from 0 to 1, so a halo
//                byte read while a neighbouring tile writes it is either value of a state on the way to the same fixed point; a
//                sweep that changes nothing has read the final state everywhere.
//   k_nav_count  the cells with reach == 1: a sum per wave, then one integer atomic per wave.
// Tiles form a one-dimensional grid (a window of one column or one row of 2^26 cells has more tiles than a grid has in y), and the
// tile shapes adapt so that such a window fills its tiles.  No workgroup waits for another; the only atomics are the counters of
// k_nav_seed and k_nav_count.
#pragma once
#include "mh_internal.h"

namespace mh {
namespace nav {

constexpr uint32_t kNavNone = 0xFFFFu, kNavFar = 0xFFFFu;
constexpr uint32_t kColCells = 4096u, kColMaxLw = 6u;    // 64 columns at most
constexpr uint32_t kColLds = kColCells + 64u * 510u;     // bytes: (2^lw) * ((4096 >> lw) + 2 Rh) never exceeds it (nav_col_lds)
constexpr uint32_t kRowCells = 256u, kRowLds = 768u;     // uint16 entries: (256 >> lw) * (2^lw + 2 Rh) < 768 (nav_row_lds)
constexpr uint32_t kReachCells = 1024u, kReachLds = 3080u;  // bytes: (2^lw + 2) * ((1024 >> lw) + 2) <= 3078

// the shapes, chosen on the host: log2 of a tile's width in cells for a window of nx x ny and a tile of `cells` cells that is
// 2^lw0 wide by default.  The tile narrows while half its width still covers nx, else widens while half its height still covers ny.
__host__ inline uint32_t nav_tile_lw(uint32_t cells_log2, uint32_t lw0, uint32_t nx, uint32_t ny) {
  uint32_t lw = lw0;
  while (lw > 0u && (1u << (lw - 1u)) >= nx) lw--;
  if (lw == lw0)
    while (lw < cells_log2 && (1u << (cells_log2 - lw - 1u)) >= ny) lw++;
  return lw;
}
__host__ inline uint32_t nav_col_lds(uint32_t lw, uint32_t Rh) { return (1u << lw) * ((kColCells >> lw) + 2u * Rh); }
__host__ inline uint32_t nav_row_lds(uint32_t lw, uint32_t Rh) { return (kRowCells >> lw) * ((1u << lw) + 2u * Rh); }
__host__ inline uint32_t nav_reach_lds(uint32_t lw) { return ((1u << lw) + 2u) * ((kReachCells >> lw) + 2u); }

// grid: ceil(nx / 2^lw) * ceil(ny / (4096 >> lw)) workgroups of 256, rows of tiles behind one another
static __global__ __launch_bounds__(256) void k_nav_col(const uint8_t* __restrict__ base, uint32_t nx, uint32_t ny, uint32_t Rh,
                                                        uint32_t unknown_is_obstacle, uint32_t lw, uint16_t* __restrict__ g) {
  __shared__ uint8_t s_ob[kColLds];
  const uint32_t CW = 1u << lw, CH = kColCells >> lw, H = CH + 2u * Rh;
  const uint32_t tiles_x = (nx + CW - 1u) >> lw, tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
  const uint32_t gx0 = tile_x << lw;
  const long long gy0 = (long long)tile_y * CH - (long long)Rh;
  for (uint32_t i = threadIdx.x; i < CW * H; i += 256u) {
    const uint32_t lx = i & (CW - 1u), ly = i >> lw;
    const uint32_t gx = gx0 + lx;
    const long long gy = gy0 + ly;
    uint8_t ob = 0;
    if (gx < nx && gy >= 0 && gy < (long long)ny) {
      const uint8_t b = base[(size_t)gy * nx + gx];
      ob = (b == 254u || (unknown_is_obstacle && b == 255u)) ? 1 : 0;
    }
    s_ob[i] = ob;  // (cells outside the window do not exist: no obstacle)
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kColCells; i += 256u) {
    const uint32_t lx = i & (CW - 1u), ly = i >> lw;
    const uint32_t gx = gx0 + lx, gy = tile_y * CH + ly;
    if (gx >= nx || gy >= ny) continue;
    const uint32_t c = ((ly + Rh) << lw) + lx;  // rows ly + Rh - d >= 0 and ly + Rh + d <= H - 1 for d <= Rh
    uint32_t out = kNavNone;
    for (uint32_t d = 0; d <= Rh; d++) {
      if (s_ob[c - (d << lw)] | s_ob[c + (d << lw)]) {
        out = d;
        break;
      }
    }
    g[(size_t)gy * nx + gx] = (uint16_t)out;
  }
}

// grid: ceil(nx / 2^lw) * ceil(ny / (256 >> lw)) workgroups of 256.  R2 = R * R.
template <bool EARLY>
static __global__ __launch_bounds__(256) void k_nav_row(const uint16_t* __restrict__ g, const uint8_t* __restrict__ base, uint32_t nx,
                                                        uint32_t ny, uint32_t R2, uint32_t Rh, uint32_t lw,
                                                        const uint8_t* __restrict__ table, uint16_t* __restrict__ d2,
                                                        uint8_t* __restrict__ cost) {
  __shared__ uint16_t s_g[kRowLds];
  const uint32_t SW = 1u << lw, RB = kRowCells >> lw, pitch = SW + 2u * Rh;
  const uint32_t segs_x = (nx + SW - 1u) >> lw, seg_x = blockIdx.x % segs_x, row0 = (blockIdx.x / segs_x) * RB;
  const long long gx0 = (long long)(seg_x << lw) - (long long)Rh;
  for (uint32_t i = threadIdx.x; i < RB * pitch; i += 256u) {
    const uint32_t r = i / pitch, lx = i - r * pitch;
    const uint32_t gy = row0 + r;
    const long long gx = gx0 + lx;
    uint16_t v = (uint16_t)kNavNone;
    if (gy < ny && gx >= 0 && gx < (long long)nx) v = g[(size_t)gy * nx + (size_t)gx];
    s_g[i] = v;
  }
  __syncthreads();
  const uint32_t lx = threadIdx.x & (SW - 1u), r = threadIdx.x >> lw;
  const uint32_t gx = (seg_x << lw) + lx, gy = row0 + r;
  if (gx >= nx || gy >= ny) return;
  const uint32_t c = r * pitch + Rh + lx;  // c - dx >= r * pitch and c + dx <= r * pitch + pitch - 1 for dx <= Rh
  uint32_t best = R2 + 1u;
  for (uint32_t dx = 0; dx <= Rh; dx++) {
    const uint32_t dd = dx * dx;
    if (EARLY && dd >= best) break;
    const uint32_t gm = min((uint32_t)s_g[c - dx], (uint32_t)s_g[c + dx]);
    if (gm != kNavNone) best = min(best, gm * gm + dd);  // (gm <= 255: the sum is below 2^17)
  }
  const size_t cell = (size_t)gy * nx + gx;
  const uint32_t b = base[cell];
  const uint32_t dist = best <= R2 ? best : kNavFar;
  d2[cell] = (uint16_t)dist;
  uint32_t out = b;
  if (b < 254u && dist != kNavFar) out = max(b, (uint32_t)table[dist]);  // (dist >= 1 here: a cell with dist 0 is an obstacle)
  cost[cell] = (uint8_t)out;
}

// ctr: {seeds on impassable cells, seeds on passable cells}
static __global__ __launch_bounds__(256) void k_nav_seed(const int* __restrict__ seeds_xy, uint32_t n_seeds, uint32_t nx, uint32_t ny,
                                                         const uint8_t* __restrict__ cost, uint32_t passable_below,
                                                         uint8_t* __restrict__ reach, uint32_t* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_seeds) return;
  const int x = seeds_xy[2u * i], y = seeds_xy[2u * i + 1u];
  if (x < 0 || y < 0 || (uint32_t)x >= nx || (uint32_t)y >= ny) return;  // (the host has counted these)
  const size_t cell = (size_t)y * nx + (size_t)x;
  if (cost[cell] < passable_below) {
    reach[cell] = 1;
    atomicAdd(&ctr[1], 1u);
  } else {
    atomicAdd(&ctr[0], 1u);
  }
}

// grid: ceil(nx / 2^lw) * ceil(ny / (1024 >> lw)) workgroups of 256, four cells per lane
static __global__ __launch_bounds__(256) void k_nav_reach(const uint8_t* __restrict__ cost, uint32_t passable_below, uint32_t nx,
                                                          uint32_t ny, uint32_t lw, uint8_t* __restrict__ reach,
                                                          uint32_t* __restrict__ flag) {
  __shared__ uint8_t s_p[kReachLds], s_r[kReachLds];
  const uint32_t TW = 1u << lw, TH = kReachCells >> lw, pitch = TW + 2u;
  const uint32_t tiles_x = (nx + TW - 1u) >> lw, tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
  const long long gx0 = (long long)(tile_x << lw) - 1, gy0 = (long long)tile_y * TH - 1;
  int seen = 0;
  for (uint32_t i = threadIdx.x; i < pitch * (TH + 2u); i += 256u) {
    const uint32_t ly = i / pitch, lx = i - ly * pitch;
    const long long gx = gx0 + lx, gy = gy0 + ly;
    uint8_t p = 0, r = 0;
    if (gx >= 0 && gy >= 0 && gx < (long long)nx && gy < (long long)ny) {
      const size_t cell = (size_t)gy * nx + (size_t)gx;
      p = cost[cell] < passable_below ? 1 : 0;
      r = reach[cell];
    }
    s_p[i] = p;
    s_r[i] = r;
    seen |= r;
  }
  if (!__syncthreads_or(seen)) return;  // nothing reached in the tile or its halo: nothing can change here
  uint32_t mine = 0;                    // bit k: this lane set its cell k
  for (;;) {
    int changed = 0;
    for (uint32_t k = 0; k < 4u; k++) {
      const uint32_t i = threadIdx.x + k * 256u;
      const uint32_t c = ((i >> lw) + 1u) * pitch + (i & (TW - 1u)) + 1u;
      if (s_p[c] && !s_r[c] && (s_r[c - 1u] | s_r[c + 1u] | s_r[c - pitch] | s_r[c + pitch])) {
        s_r[c] = 1;
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
    reach[(size_t)gy * nx + gx] = 1;
  }
  *flag = 1u;
}

static __global__ __launch_bounds__(256) void k_nav_count(const uint8_t* __restrict__ reach, size_t n, uint32_t* __restrict__ total) {
  uint32_t sum = 0;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) sum += reach[i];
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(total, sum);
}

}  // namespace nav
}  // namespace mh
