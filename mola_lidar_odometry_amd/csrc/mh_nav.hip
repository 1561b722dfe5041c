// mh_nav.hip -- the entry points of include/molahip_nav.h: the base plane, the two passes of the distance
// transform with the inflated cost, the flood fill of the reachable region as a host loop of sweeps, and the download.  The reading
// is written down in the header; the kernels are mh_k_nav.h's.
#include <new>

#include "../../include/molahip_nav.h"
#include "mh_k_nav.h"
#include "mh_nav_internal.h"

using namespace mh;
using namespace mh::nav;

namespace {
inline uint32_t nblk(size_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }
}  // namespace

extern "C" {

uint32_t mh_nav_api_version(void) { return MH_NAV_API_VERSION; }

mh_status mh_nav_create(mh_ctx* ctx, uint32_t nx, uint32_t ny, mh_nav** out) {
  MH_REQUIRE(ctx && out, "null argument");
  MH_REQUIRE(nx > 0 && ny > 0, "nx and ny must be > 0");
  MH_REQUIRE((uint64_t)nx * (uint64_t)ny <= (1ull << 26), "nx * ny must not exceed 2^26");
  MH_TRY(set_device(ctx));
  mh_nav* n = new (std::nothrow) mh_nav();
  if (!n) return fail(MH_ERR_OUT_OF_MEMORY, "mh_nav_create: out of host memory");
  n->ctx = ctx;
  n->nx = nx;
  n->ny = ny;
  n->n_cells = (size_t)nx * ny;
  n->stride = (n->n_cells + 255) / 256 * 256;
  n->info.nx = nx;
  n->info.ny = ny;
  mh_status st = n->bytes.reserve(3 * n->stride);
  if (st == MH_OK) st = n->words.reserve(2 * n->stride * sizeof(uint16_t));
  if (st == MH_OK) st = n->ctr.reserve(4 * sizeof(uint32_t));
  if (st == MH_OK) st = n->h_ctr.reserve(4 * sizeof(uint32_t));
  if (st != MH_OK) {
    (void)mh_nav_destroy(n);
    return st;
  }
  *out = n;
  return MH_OK;
}

mh_status mh_nav_destroy(mh_nav* n) {
  if (!n) return MH_OK;
  (void)set_device(n->ctx);
  (void)mh::wait_stream(n->ctx->stream);
  n->bytes.release();
  n->words.release();
  n->table.release();
  n->seeds.release();
  n->ctr.release();
  n->h_ctr.release();
  delete n;
  return MH_OK;
}

mh_status mh_nav_get_info(const mh_nav* n, mh_nav_info* info) {
  MH_REQUIRE(n && info, "null argument");
  *info = n->info;
  return MH_OK;
}

mh_status mh_nav_set_base(mh_nav* n, const uint8_t* bytes, int32_t mem) {
  MH_REQUIRE(n && bytes, "null argument");
  MH_REQUIRE(mem == MH_MEM_HOST || mem == MH_MEM_DEVICE || mem == MH_MEM_HOST_PINNED, "bad mem");
  MH_TRY(set_device(n->ctx));
  hipStream_t s = n->ctx->stream;
  n->info.has_base = n->info.has_cost = n->info.has_reach = 0u;
  n->info.n_reached = n->info.n_seeds_blocked = n->info.n_seeds_outside = 0;
  n->info.n_sweeps = 0;
  MH_HIP(hipMemcpyAsync(n->base(), bytes, n->n_cells, mem == MH_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  MH_HIP(mh::wait_stream(s));  // (the caller's array is free again behind this)
  n->info.has_base = 1u;
  return MH_OK;
}

mh_status mh_nav_inflate(mh_nav* n, uint32_t max_cells, int32_t unknown_is_obstacle, const uint8_t* table, size_t n_table) {
  MH_REQUIRE(n && table, "null argument");
  MH_REQUIRE(max_cells <= MH_NAV_MAX_CELLS, "max_cells must not exceed 255");
  MH_REQUIRE(n_table == (size_t)max_cells * max_cells + 1, "n_table must be max_cells * max_cells + 1");
  for (size_t k = 0; k < n_table; k++) MH_REQUIRE(table[k] <= MH_NAV_MAX_TABLE, "a table entry exceeds 253");
  MH_REQUIRE(n->info.has_base, "no base plane: mh_nav_set_base comes first");
  const Switches sw = read_switches();
  const uint32_t R = max_cells, nx = n->nx, ny = n->ny;
  const uint32_t Rv = std::min(R, ny - 1u), Rh = std::min(R, nx - 1u);  // (cells beyond the window do not exist)
  const uint32_t lw_col = nav_tile_lw(12u, kColMaxLw, nx, ny), lw_row = nav_tile_lw(8u, 8u, nx, ny);
  if (nav_col_lds(lw_col, Rv) > kColLds || nav_row_lds(lw_row, Rh) > kRowLds)
    return fail(MH_ERR_INTERNAL, "mh_nav_inflate: a tile of %u x %u cells does not fit its LDS image", nx, ny);
  MH_TRY(set_device(n->ctx));
  hipStream_t s = n->ctx->stream;
  n->info.has_cost = n->info.has_reach = 0u;
  MH_TRY(n->table.reserve(n_table));
  MH_HIP(hipMemcpyAsync(n->table.p, table, n_table, hipMemcpyHostToDevice, s));
  const uint32_t col_tiles = nblk(nx, 1u << lw_col) * nblk(ny, kColCells >> lw_col);
  hipLaunchKernelGGL(k_nav_col, dim3(col_tiles), dim3(256), 0, s, n->base(), nx, ny, Rv, unknown_is_obstacle ? 1u : 0u, lw_col, n->g());
  MH_HIP(hipGetLastError());
  const uint32_t row_tiles = nblk(nx, 1u << lw_row) * nblk(ny, kRowCells >> lw_row);
  if (sw.nav_no_early_stop)
    hipLaunchKernelGGL(k_nav_row<false>, dim3(row_tiles), dim3(256), 0, s, n->g(), n->base(), nx, ny, R * R, Rh, lw_row,
                       n->table.as<uint8_t>(), n->d2(), n->cost());
  else
    hipLaunchKernelGGL(k_nav_row<true>, dim3(row_tiles), dim3(256), 0, s, n->g(), n->base(), nx, ny, R * R, Rh, lw_row,
                       n->table.as<uint8_t>(), n->d2(), n->cost());
  MH_HIP(hipGetLastError());
  MH_HIP(mh::wait_stream(s));  // (the caller's table is free again behind this)
  n->info.max_cells = R;
  n->info.has_cost = 1u;
  return MH_OK;
}

mh_status mh_nav_reach(mh_nav* n, const int32_t* seeds_xy, size_t n_seeds, uint32_t passable_below) {
  MH_REQUIRE(n, "null argument");
  MH_REQUIRE(seeds_xy || n_seeds == 0, "null seeds with n_seeds > 0");
  MH_REQUIRE(n_seeds <= 0x7FFFFFF0ull, "too many seeds");
  MH_REQUIRE(passable_below >= 1u && passable_below <= 254u, "passable_below must lie in 1 .. 254");
  MH_REQUIRE(n->info.has_cost, "no cost plane: mh_nav_inflate comes first");
  const uint32_t nx = n->nx, ny = n->ny;
  const uint32_t lw = nav_tile_lw(10u, 6u, nx, ny);
  if (nav_reach_lds(lw) > kReachLds) return fail(MH_ERR_INTERNAL, "mh_nav_reach: a tile of %u x %u cells does not fit its LDS image", nx, ny);
  MH_TRY(set_device(n->ctx));
  hipStream_t s = n->ctx->stream;
  n->info.has_reach = 0u;
  uint64_t outside = 0;
  for (size_t k = 0; k < n_seeds; k++) {
    const int32_t x = seeds_xy[2 * k], y = seeds_xy[2 * k + 1];
    if (x < 0 || y < 0 || (uint32_t)x >= nx || (uint32_t)y >= ny) outside++;
  }
  uint32_t* d_ctr = n->ctr.as<uint32_t>();
  uint32_t* h_ctr = n->h_ctr.as<uint32_t>();
  MH_HIP(hipMemsetAsync(n->reach(), 0, n->n_cells, s));
  MH_HIP(hipMemsetAsync(d_ctr, 0, 4 * sizeof(uint32_t), s));
  uint32_t sweeps = 0;
  h_ctr[0] = h_ctr[1] = h_ctr[2] = h_ctr[3] = 0u;
  if (n_seeds > outside) {
    MH_TRY(n->seeds.reserve(n_seeds * 2 * sizeof(int32_t)));
    MH_HIP(hipMemcpyAsync(n->seeds.p, seeds_xy, n_seeds * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_nav_seed, dim3(nblk(n_seeds, 256)), dim3(256), 0, s, n->seeds.as<int>(), (uint32_t)n_seeds, nx, ny, n->cost(),
                       passable_below, n->reach(), d_ctr);
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(h_ctr, d_ctr, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));  // (the caller's seeds are free again behind this)
    if (h_ctr[1]) {
      // The set only grows and is bounded by the passable cells, so a sweep that changes nothing comes; every sweep is a launch of
      // its own and the host reads its flag: no workgroup ever waits for another.
      const uint32_t tiles = nblk(nx, 1u << lw) * nblk(ny, kReachCells >> lw);
      for (;;) {
        MH_HIP(hipMemsetAsync(d_ctr + 3, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_nav_reach, dim3(tiles), dim3(256), 0, s, n->cost(), passable_below, nx, ny, lw, n->reach(), d_ctr + 3);
        MH_HIP(hipGetLastError());
        MH_HIP(hipMemcpyAsync(h_ctr + 3, d_ctr + 3, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        MH_HIP(mh::wait_stream(s));
        sweeps++;
        if (!h_ctr[3]) break;
        // (every sweep that changes something adds a cell: more sweeps than cells cannot be)
        if ((uint64_t)sweeps > (uint64_t)n->n_cells) return fail(MH_ERR_INTERNAL, "mh_nav_reach: the sweeps do not come to rest");
      }
      hipLaunchKernelGGL(k_nav_count, dim3(std::min<uint32_t>(nblk(n->n_cells, 256), 4096u)), dim3(256), 0, s, n->reach(), n->n_cells,
                         d_ctr + 2);
      MH_HIP(hipGetLastError());
      MH_HIP(hipMemcpyAsync(h_ctr + 2, d_ctr + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
  }
  MH_HIP(mh::wait_stream(s));
  n->info.n_seeds_outside = outside;
  n->info.n_seeds_blocked = h_ctr[0];
  n->info.n_reached = h_ctr[2];
  n->info.n_sweeps = sweeps;
  n->info.has_reach = 1u;
  return MH_OK;
}

mh_status mh_nav_download(const mh_nav* n, uint16_t* d2, uint8_t* cost, uint8_t* reach) {
  MH_REQUIRE(n, "null argument");
  MH_REQUIRE(!(d2 || cost) || n->info.has_cost, "d2 and cost have not been computed since the last mh_nav_set_base");
  MH_REQUIRE(!reach || n->info.has_reach, "reach has not been computed since the last mh_nav_set_base");
  MH_TRY(set_device(n->ctx));
  hipStream_t s = n->ctx->stream;
  if (d2) MH_HIP(hipMemcpyAsync(d2, n->d2(), n->n_cells * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
  if (cost) MH_HIP(hipMemcpyAsync(cost, n->cost(), n->n_cells, hipMemcpyDeviceToHost, s));
  if (reach) MH_HIP(hipMemcpyAsync(reach, n->reach(), n->n_cells, hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  return MH_OK;
}

}  // extern "C"
