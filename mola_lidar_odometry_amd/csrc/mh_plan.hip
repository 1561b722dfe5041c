// mh_plan.hip -- the entry points of include/molahip_plan.h: the cost plane, the cost-to-go field as a host loop
// of sweeps over the active tiles, the route trace and the download.  The reading is written down in the header; the kernels are
// mh_k_plan.h's.
#include <new>
#include <vector>

#include "../../include/molahip_plan.h"
#include "mh_k_plan.h"
#include "mh_nav_internal.h"
#include "mh_plan_internal.h"

using namespace mh;
using namespace mh::nav;
using namespace mh::plan;

namespace mh {
namespace plan {

mh_status relax_to_rest(mh_plan* p, bool all_tiles, uint8_t* first, uint32_t* sweeps, uint64_t* tile_runs) {
  // Values only fall and are bounded below, so a sweep that changes nothing comes; every sweep is a launch of its own and the
  // host reads its flag: no workgroup ever waits for another.  `prev` holds the tiles that changed in the sweep before.
  hipStream_t s = p->ctx->stream;
  uint32_t* d_ctr = p->ctr.as<uint32_t>();
  uint32_t* h_ctr = p->h_ctr.as<uint32_t>();
  uint8_t* prev = first;
  uint8_t* now = first == p->plane(0) ? p->plane(1) : p->plane(0);
  uint64_t mine = 0;
  for (;;) {
    MH_HIP(hipMemsetAsync(d_ctr + 4, 0, 2 * sizeof(uint32_t), s));
    MH_HIP(hipMemsetAsync(now, 0, p->n_tiles, s));
    hipLaunchKernelGGL(k_plan_relax, dim3(p->n_tiles), dim3(256), 0, s, p->cost.as<uint8_t>(), p->price.as<uint16_t>(), p->nx, p->ny, p->lw,
                       all_tiles ? 1u : 0u, prev, now, p->field.as<uint32_t>(), d_ctr + 4);
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(h_ctr + 4, d_ctr + 4, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));
    (*sweeps)++;
    mine++;
    *tile_runs += h_ctr[5];
    prev = now;
    now = now == p->plane(0) ? p->plane(1) : p->plane(0);
    if (!h_ctr[4]) break;
    // (Bellman-Ford: after k sweeps every cell whose cheapest route has k steps is final, so more changing sweeps than cells
    // cannot be)
    if (mine > (uint64_t)p->n_cells) return fail(MH_ERR_INTERNAL, "mh_plan_field: the sweeps do not come to rest");
  }
  return MH_OK;
}

mh_status field_from_goals(mh_plan* p, const Switches& sw, uint32_t passable_below) {
  hipStream_t s = p->ctx->stream;
  uint32_t* d_ctr = p->ctr.as<uint32_t>();
  uint32_t* h_ctr = p->h_ctr.as<uint32_t>();
  for (uint32_t k = 0; k < 8u; k++) h_ctr[k] = 0u;
  MH_HIP(hipMemsetAsync(p->field.p, 0xFF, p->n_cells * sizeof(uint32_t), s));
  MH_HIP(hipMemsetAsync(d_ctr, 0, 8 * sizeof(uint32_t), s));
  MH_HIP(hipMemsetAsync(p->changed.p, 0, 2 * p->tile_stride, s));
  uint32_t sweeps = 0;
  uint64_t tile_runs = 0;
  if (p->n_goals > p->info.n_goals_outside) {
    hipLaunchKernelGGL(k_plan_goals, dim3(nblk(p->n_goals, 256)), dim3(256), 0, s, p->goals.as<int>(), (uint32_t)p->n_goals, p->nx, p->ny,
                       p->cost.as<uint8_t>(), passable_below, p->lw, p->field.as<uint32_t>(), p->plane(0), d_ctr);
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(h_ctr, d_ctr, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));
    if (h_ctr[1]) {
      MH_TRY(relax_to_rest(p, sw.plan_all_tiles, p->plane(0), &sweeps, &tile_runs));
      hipLaunchKernelGGL(k_plan_stats, dim3(std::min<uint32_t>(nblk(p->n_cells, 256), 4096u)), dim3(256), 0, s, p->field.as<uint32_t>(),
                         p->n_cells, d_ctr + 2);
      MH_HIP(hipGetLastError());
      MH_HIP(hipMemcpyAsync(h_ctr + 2, d_ctr + 2, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
  }
  MH_HIP(mh::wait_stream(s));
  p->info.n_goals_blocked = h_ctr[0];
  p->info.n_reached = h_ctr[2];
  p->info.max_field = h_ctr[3];
  p->info.n_sweeps = sweeps;
  p->info.n_tile_runs = tile_runs;
  p->info.passable_below = passable_below;
  p->info.has_field = 1u;
  return MH_OK;
}

}  // namespace plan
}  // namespace mh

extern "C" {

uint32_t mh_plan_api_version(void) { return MH_PLAN_API_VERSION; }

mh_status mh_plan_create(mh_ctx* ctx, uint32_t nx, uint32_t ny, mh_plan** out) {
  MH_REQUIRE(ctx && out, "null argument");
  MH_REQUIRE(nx > 0 && ny > 0, "nx and ny must be > 0");
  MH_REQUIRE((uint64_t)nx * (uint64_t)ny <= (1ull << 26), "nx * ny must not exceed 2^26");
  MH_TRY(set_device(ctx));
  mh_plan* p = new (std::nothrow) mh_plan();
  if (!p) return fail(MH_ERR_OUT_OF_MEMORY, "mh_plan_create: out of host memory");
  p->ctx = ctx;
  p->nx = nx;
  p->ny = ny;
  p->n_cells = (size_t)nx * ny;
  p->lw = nav_tile_lw(10u, 6u, nx, ny);
  p->n_tiles = nblk(nx, 1u << p->lw) * nblk(ny, kPlanCells >> p->lw);
  p->tile_stride = ((size_t)p->n_tiles + 255) / 256 * 256;
  p->info.nx = nx;
  p->info.ny = ny;
  mh_status st = p->cost.reserve(p->n_cells);
  if (st == MH_OK) st = p->field.reserve(p->n_cells * sizeof(uint32_t));
  if (st == MH_OK) st = p->price.reserve(256 * sizeof(uint16_t));
  if (st == MH_OK) st = p->changed.reserve(3 * p->tile_stride);
  if (st == MH_OK) st = p->ctr.reserve(kCtrs * sizeof(uint32_t));
  if (st == MH_OK) st = p->h_ctr.reserve(kCtrs * sizeof(uint32_t) + 256 * sizeof(uint16_t));
  if (st != MH_OK) {
    (void)mh_plan_destroy(p);
    return st;
  }
  *out = p;
  return MH_OK;
}

mh_status mh_plan_destroy(mh_plan* p) {
  if (!p) return MH_OK;
  (void)set_device(p->ctx);
  (void)mh::wait_stream(p->ctx->stream);
  p->cost.release();
  p->field.release();
  p->price.release();
  p->goals.release();
  p->patch.release();
  p->changed.release();
  p->ctr.release();
  p->h_ctr.release();
  p->t_starts.release();
  p->t_out.release();
  p->t_len.release();
  delete p;
  return MH_OK;
}

mh_status mh_plan_get_info(const mh_plan* p, mh_plan_info* info) {
  MH_REQUIRE(p && info, "null argument");
  *info = p->info;
  return MH_OK;
}

mh_status mh_plan_set_cost(mh_plan* p, const uint8_t* bytes, int32_t mem) {
  MH_REQUIRE(p && bytes, "null argument");
  MH_REQUIRE(mem == MH_MEM_HOST || mem == MH_MEM_DEVICE || mem == MH_MEM_HOST_PINNED, "bad mem");
  MH_TRY(set_device(p->ctx));
  hipStream_t s = p->ctx->stream;
  p->info.has_cost = 0u;
  forget_field(p);
  MH_HIP(hipMemcpyAsync(p->cost.p, bytes, p->n_cells, mem == MH_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  MH_HIP(mh::wait_stream(s));  // (the caller's array is free again behind this)
  p->info.has_cost = 1u;
  return MH_OK;
}

mh_status mh_plan_set_cost_from_nav(mh_plan* p, const mh_nav* nav) {
  MH_REQUIRE(p && nav, "null argument");
  MH_REQUIRE(nav->info.has_cost, "the mh_nav holds no cost plane: mh_nav_inflate comes first");
  MH_REQUIRE(nav->nx == p->nx && nav->ny == p->ny, "the mh_nav's window is not the plan's");
  MH_REQUIRE(nav->ctx == p->ctx, "the mh_nav was created on another context");
  return mh_plan_set_cost(p, nav->cost(), MH_MEM_DEVICE);
}

mh_status mh_plan_field(mh_plan* p, const int32_t* goals_xy, size_t n_goals, uint32_t passable_below, const uint16_t* price, size_t n_price) {
  MH_REQUIRE(p && price, "null argument");
  MH_REQUIRE(goals_xy || n_goals == 0, "null goals with n_goals > 0");
  MH_REQUIRE(n_goals <= 0x7FFFFFF0ull, "too many goals");
  MH_REQUIRE(passable_below >= 1u && passable_below <= 254u, "passable_below must lie in 1 .. 254");
  MH_REQUIRE(n_price == (size_t)passable_below, "n_price must be passable_below");
  uint64_t top = 0;
  for (size_t k = 0; k < n_price; k++) {
    MH_REQUIRE(price[k] >= 1u, "a price of 0");
    top = std::max<uint64_t>(top, price[k]);
  }
  // no finite value can pass (n_cells - 1) steps of at most 14 * max(price) each
  MH_REQUIRE((uint64_t)(p->n_cells - 1) * 14ull * top < 0xFFFFFFFFull, "(nx * ny - 1) * 14 * max(price) does not stay below 2^32 - 1: the field could wrap round");
  MH_REQUIRE(p->info.has_cost, "no cost plane: mh_plan_set_cost comes first");
  const Switches sw = read_switches();
  const uint32_t nx = p->nx, ny = p->ny, lw = p->lw;
  if (nav_reach_lds(lw) > kPlanLds) return fail(MH_ERR_INTERNAL, "mh_plan_field: a tile of %u x %u cells does not fit its LDS image", nx, ny);
  MH_TRY(set_device(p->ctx));
  hipStream_t s = p->ctx->stream;
  forget_field(p);
  uint64_t outside = 0;
  for (size_t k = 0; k < n_goals; k++) {
    const int32_t x = goals_xy[2 * k], y = goals_xy[2 * k + 1];
    if (x < 0 || y < 0 || (uint32_t)x >= nx || (uint32_t)y >= ny) outside++;
  }
  uint16_t* h_price = reinterpret_cast<uint16_t*>(p->h_ctr.as<uint32_t>() + kCtrs);  // (behind the counters in the pinned block)
  for (uint32_t k = 0; k < 256u; k++) h_price[k] = k < passable_below ? price[k] : (uint16_t)0;
  MH_HIP(hipMemcpyAsync(p->price.p, h_price, 256 * sizeof(uint16_t), hipMemcpyHostToDevice, s));
  p->n_goals = 0;
  if (n_goals > outside) {
    MH_TRY(p->goals.reserve(n_goals * 2 * sizeof(int32_t)));
    MH_HIP(hipMemcpyAsync(p->goals.p, goals_xy, n_goals * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    MH_HIP(mh::wait_stream(s));  // (the caller's goals are free again behind this)
    p->n_goals = n_goals;
  }
  p->info.n_goals_outside = outside;
  const mh_status st = field_from_goals(p, sw, passable_below);
  if (st != MH_OK) forget_field(p);
  return st;
}

mh_status mh_plan_trace(const mh_plan* p, const int32_t* starts_xy, size_t n_starts, uint32_t cap, int32_t* out_xy, uint32_t* out_len) {
  MH_REQUIRE(p, "null argument");
  MH_REQUIRE(n_starts == 0 || (starts_xy && out_xy && out_len), "null starts, out_xy or out_len with n_starts > 0");
  MH_REQUIRE(n_starts <= 0x7FFFFFF0ull, "too many starts");
  MH_REQUIRE(cap >= 1u, "cap must be >= 1");
  MH_REQUIRE(p->info.has_field, "no field: mh_plan_field comes first");
  if (n_starts == 0) return MH_OK;
  MH_TRY(set_device(p->ctx));
  hipStream_t s = p->ctx->stream;
  // (a route visits a cell at most once: no more than n_cells pairs per start are ever written)
  const uint32_t dcap = (uint32_t)std::min<uint64_t>(cap, p->n_cells);
  const size_t n_pairs = n_starts * (size_t)dcap;
  MH_TRY(p->t_starts.reserve(n_starts * 2 * sizeof(int32_t)));
  MH_TRY(p->t_out.reserve(n_pairs * 2 * sizeof(int32_t)));
  MH_TRY(p->t_len.reserve(n_starts * sizeof(uint32_t)));
  MH_HIP(hipMemcpyAsync(p->t_starts.p, starts_xy, n_starts * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_plan_trace, dim3(nblk(n_starts, 4)), dim3(256), 0, s, p->cost.as<uint8_t>(), p->price.as<uint16_t>(),
                     p->field.as<uint32_t>(), p->nx, p->ny, p->t_starts.as<int>(), (uint32_t)n_starts, dcap, p->t_out.as<int>(),
                     p->t_len.as<uint32_t>());
  MH_HIP(hipGetLastError());
  MH_HIP(hipMemcpyAsync(out_len, p->t_len.p, n_starts * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  for (size_t i = 0; i < n_starts; i++) {  // each route's own cells, to where the caller's `cap` puts them
    const size_t n = out_len[i] == MH_PLAN_TRUNCATED ? dcap : out_len[i];
    if (n) MH_HIP(hipMemcpyAsync(out_xy + i * (size_t)cap * 2, p->t_out.as<int>() + i * (size_t)dcap * 2, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  }
  MH_HIP(mh::wait_stream(s));
  return MH_OK;
}

mh_status mh_plan_download(const mh_plan* p, uint32_t* field) {
  MH_REQUIRE(p && field, "null argument");
  MH_REQUIRE(p->info.has_field, "no field: mh_plan_field comes first");
  MH_TRY(set_device(p->ctx));
  hipStream_t s = p->ctx->stream;
  MH_HIP(hipMemcpyAsync(field, p->field.p, p->n_cells * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  return MH_OK;
}

}  // extern "C"
