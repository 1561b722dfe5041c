// mh_replan.hip -- the entry points of include/molahip_replan.h: a rectangle of new cost bytes, the withdrawal of
// the field values that rested on what it took away, and mh_plan_field's relax loop from the tiles that were touched.  The reading is
// written down in the header; the kernels are mh_k_replan.h's and mh_k_plan.h's, the handle and the relax loop mh_plan_internal.h's.
#include "../../include/molahip_replan.h"
#include "mh_k_replan.h"
#include "mh_nav_internal.h"
#include "mh_plan_internal.h"

using namespace mh;
using namespace mh::nav;
using namespace mh::plan;

namespace {

// `src` is on the device: row r of the rectangle at src + r * pitch.
mh_status update(mh_plan* p, const uint8_t* src, size_t pitch, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const Switches& sw) {
  hipStream_t s = p->ctx->stream;
  const uint32_t nx = p->nx, ny = p->ny, lw = p->lw;
  uint32_t* d_ctr = p->ctr.as<uint32_t>();
  uint32_t* h_ctr = p->h_ctr.as<uint32_t>();
  const bool with_field = p->info.has_field != 0u;
  const uint32_t below = p->info.passable_below;
  mh_replan_info r{};
  r.n_updates = p->rinfo.n_updates + 1u;
  MH_HIP(hipMemsetAsync(d_ctr + 8, 0, 3 * sizeof(uint32_t), s));
  if (with_field) MH_HIP(hipMemsetAsync(p->changed.p, 0, 3 * p->tile_stride, s));
  hipLaunchKernelGGL(k_replan_patch, dim3(nblk((size_t)w * h, 256)), dim3(256), 0, s, src, pitch, x0, y0, w, h, nx, ny, lw,
                     p->price.as<uint16_t>(), p->cost.as<uint8_t>(), with_field ? p->field.as<uint32_t>() : nullptr, p->plane(0), p->plane(2),
                     d_ctr + 8);
  MH_HIP(hipGetLastError());
  MH_HIP(hipMemcpyAsync(h_ctr + 8, d_ctr + 8, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));  // (the caller's array is free again behind this)
  r.n_cells_changed = h_ctr[8];
  r.n_cells_repriced = h_ctr[9];
  p->rinfo = r;
  if (!with_field) return MH_OK;
  p->info.n_sweeps = 0u;
  p->info.n_tile_runs = 0;
  if (!r.n_cells_repriced) return MH_OK;  // no step weight and no passability changed: the field stands
  if (sw.replan_full) {
    MH_TRY(field_from_goals(p, sw, below));
    p->rinfo.n_relax_sweeps = p->info.n_sweeps;
    p->rinfo.n_tile_runs_relax = p->info.n_tile_runs;
    return MH_OK;
  }
  if (!(p->n_goals > p->info.n_goals_outside)) return MH_OK;  // no goal inside the window: all UNREACHED before and after
  // 1. withdraw.  Values only go from finite to UNREACHED, so a sweep that changes nothing comes; every sweep is a launch of its own
  // and the host reads its flag.  plane 0 holds the patch's tiles, plane 2 gathers every tile that is touched.
  uint64_t withdrawn = h_ctr[10];
  {
    uint8_t* prev = p->plane(0);
    uint8_t* now = p->plane(1);
    for (;;) {
      MH_HIP(hipMemsetAsync(d_ctr + 4, 0, 3 * sizeof(uint32_t), s));
      MH_HIP(hipMemsetAsync(now, 0, p->n_tiles, s));
      hipLaunchKernelGGL(k_replan_withdraw, dim3(p->n_tiles), dim3(256), 0, s, p->cost.as<uint8_t>(), p->price.as<uint16_t>(), nx, ny, lw,
                         sw.plan_all_tiles ? 1u : 0u, prev, now, p->plane(2), p->field.as<uint32_t>(), d_ctr + 4);
      MH_HIP(hipGetLastError());
      MH_HIP(hipMemcpyAsync(h_ctr + 4, d_ctr + 4, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      MH_HIP(mh::wait_stream(s));
      r.n_withdraw_sweeps++;
      r.n_tile_runs_withdraw += h_ctr[5];
      withdrawn += h_ctr[6];
      std::swap(prev, now);
      if (!h_ctr[4]) break;
      // (every changing sweep takes at least one cell back for good)
      if ((uint64_t)r.n_withdraw_sweeps > (uint64_t)p->n_cells) return fail(MH_ERR_INTERNAL, "mh_replan_update_cost: the withdraw sweeps do not come to rest");
    }
  }
  r.n_withdrawn = withdrawn;
  // 2. the goals again, by mh_plan_field's rule: 0 into a passable goal cell, the counts, the flags -- into the touched plane
  for (uint32_t k = 0; k < 4u; k++) h_ctr[k] = 0u;
  MH_HIP(hipMemsetAsync(d_ctr, 0, 4 * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_plan_goals, dim3(nblk(p->n_goals, 256)), dim3(256), 0, s, p->goals.as<int>(), (uint32_t)p->n_goals, nx, ny,
                     p->cost.as<uint8_t>(), below, lw, p->field.as<uint32_t>(), p->plane(2), d_ctr);
  MH_HIP(hipGetLastError());
  MH_HIP(hipMemcpyAsync(h_ctr, d_ctr, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  // 3. relax from the touched tiles, 4. the statistics
  uint32_t sweeps = 0;
  uint64_t tile_runs = 0;
  if (h_ctr[1]) {
    MH_TRY(relax_to_rest(p, sw.plan_all_tiles, p->plane(2), &sweeps, &tile_runs));
    hipLaunchKernelGGL(k_plan_stats, dim3(std::min<uint32_t>(nblk(p->n_cells, 256), 4096u)), dim3(256), 0, s, p->field.as<uint32_t>(), p->n_cells,
                       d_ctr + 2);
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(h_ctr + 2, d_ctr + 2, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));
  }
  r.n_relax_sweeps = sweeps;
  r.n_tile_runs_relax = tile_runs;
  p->info.n_goals_blocked = h_ctr[0];
  p->info.n_reached = h_ctr[2];
  p->info.max_field = h_ctr[3];
  p->info.n_sweeps = sweeps;
  p->info.n_tile_runs = tile_runs;
  p->rinfo = r;
  return MH_OK;
}

// a failure half-way leaves no field behind
mh_status update_or_forget(mh_plan* p, const uint8_t* src, size_t pitch, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const Switches& sw) {
  const mh_status st = update(p, src, pitch, x0, y0, w, h, sw);
  if (st != MH_OK) forget_field(p);
  return st;
}

bool rect_inside(const mh_plan* p, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
  return (uint64_t)x0 + (uint64_t)w <= (uint64_t)p->nx && (uint64_t)y0 + (uint64_t)h <= (uint64_t)p->ny;
}

}  // namespace

extern "C" {

uint32_t mh_replan_api_version(void) { return MH_REPLAN_API_VERSION; }

mh_status mh_replan_get_info(const mh_plan* p, mh_replan_info* info) {
  MH_REQUIRE(p && info, "null argument");
  *info = p->rinfo;
  return MH_OK;
}

mh_status mh_replan_update_cost(mh_plan* p, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const uint8_t* bytes, int32_t mem) {
  MH_REQUIRE(p && bytes, "null argument");
  MH_REQUIRE(mem == MH_MEM_HOST || mem == MH_MEM_DEVICE || mem == MH_MEM_HOST_PINNED, "bad mem");
  MH_REQUIRE(w > 0 && h > 0, "w and h must be > 0");
  MH_REQUIRE(rect_inside(p, x0, y0, w, h), "the rectangle does not lie inside the window");
  MH_REQUIRE(p->info.has_cost, "no cost plane: mh_plan_set_cost comes first");
  const Switches sw = read_switches();
  if (nav_reach_lds(p->lw) > kPlanLds) return fail(MH_ERR_INTERNAL, "mh_replan_update_cost: a tile of %u x %u cells does not fit its LDS image", p->nx, p->ny);
  MH_TRY(set_device(p->ctx));
  const uint8_t* src = bytes;
  if (mem != MH_MEM_DEVICE) {
    MH_TRY(p->patch.reserve((size_t)w * h));
    MH_HIP(hipMemcpyAsync(p->patch.p, bytes, (size_t)w * h, hipMemcpyHostToDevice, p->ctx->stream));
    src = p->patch.as<uint8_t>();
  }
  return update_or_forget(p, src, w, x0, y0, w, h, sw);
}

mh_status mh_replan_update_cost_from_nav(mh_plan* p, const mh_nav* nav, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
  MH_REQUIRE(p && nav, "null argument");
  MH_REQUIRE(w > 0 && h > 0, "w and h must be > 0");
  MH_REQUIRE(rect_inside(p, x0, y0, w, h), "the rectangle does not lie inside the window");
  MH_REQUIRE(p->info.has_cost, "no cost plane: mh_plan_set_cost comes first");
  MH_REQUIRE(nav->info.has_cost, "the mh_nav holds no cost plane: mh_nav_inflate comes first");
  MH_REQUIRE(nav->nx == p->nx && nav->ny == p->ny, "the mh_nav's window is not the plan's");
  MH_REQUIRE(nav->ctx == p->ctx, "the mh_nav was created on another context");
  const Switches sw = read_switches();
  if (nav_reach_lds(p->lw) > kPlanLds) return fail(MH_ERR_INTERNAL, "mh_replan_update_cost_from_nav: a tile of %u x %u cells does not fit its LDS image", p->nx, p->ny);
  MH_TRY(set_device(p->ctx));
  return update_or_forget(p, nav->cost() + (size_t)y0 * p->nx + x0, p->nx, x0, y0, w, h, sw);
}

}  // extern "C"
