// mh_plan_internal.h -- the body of the plan handle and the two steps that mh_plan.hip (mh_plan_field) and mh_replan.hip (the updates
// of include/molahip_replan.h) share: the relax loop and the whole field from the goals kept on the device.
#pragma once
#include "../../include/molahip_plan.h"
#include "../../include/molahip_replan.h"
#include "mh_internal.h"
#include "mh_switches.h"

struct mh_plan {
  mh_ctx* ctx = nullptr;
  uint32_t nx = 0, ny = 0;
  size_t n_cells = 0;
  uint32_t lw = 0, n_tiles = 0;  // the relax tiles: 2^lw cells wide
  mh::DevBuf cost;     // n_cells bytes
  mh::DevBuf field;    // n_cells uint32
  mh::DevBuf price;    // uint16 [256] of the last field: 0 = impassable
  mh::DevBuf goals;    // the goals of the last field
  size_t n_goals = 0;  // ... and their number
  mh::DevBuf changed;  // three byte planes of n_tiles flags (256-byte aligned sections): two the sweeps alternate between, and the
                       // tiles an update touched
  mh::DevBuf ctr;      // uint32 [16]: goals blocked, goals placed, cells reached, max field, the sweep's flag, the sweep's tile runs,
                       // the sweep's withdrawn cells, -, an update's cells changed, repriced, closed with a finite field
  mh::PinnedBuf h_ctr;  // ... their mirror, and the price table on its way up behind them
  mh::DevBuf patch;     // an update's rectangle on its way up
  mutable mh::DevBuf t_starts, t_out, t_len;  // mh_plan_trace's scratch
  size_t tile_stride = 0;
  mh_plan_info info{};
  mh_replan_info rinfo{};
  uint8_t* plane(uint32_t k) const { return changed.as<uint8_t>() + k * tile_stride; }
};

namespace mh {
namespace plan {

constexpr uint32_t kCtrs = 16u;

inline uint32_t nblk(size_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// no field any more: what mh_plan_set_cost, a new mh_plan_field and a failure half-way through a field or an update leave
inline void forget_field(mh_plan* p) {
  p->info.has_field = 0u;
  p->info.n_reached = p->info.n_goals_blocked = p->info.n_goals_outside = p->info.n_tile_runs = 0;
  p->info.n_sweeps = p->info.max_field = p->info.passable_below = 0u;
  p->rinfo = mh_replan_info{};
}

// Sweeps of k_plan_relax until one changes nothing.  `first` is the plane of the tiles that count as changed before the first sweep
// (plane 0 or plane 2); the sweeps then alternate between planes 0 and 1.  Adds to *sweeps and *tile_runs.
mh_status relax_to_rest(mh_plan* p, bool all_tiles, uint8_t* first, uint32_t* sweeps, uint64_t* tile_runs);

// The whole field from nothing for the goals, passable_below and prices the handle keeps on the device (p->goals, p->n_goals,
// p->price): what mh_plan_field does behind its uploads.  Fills every counter of p->info but n_goals_outside and passable_below and
// sets has_field.
mh_status field_from_goals(mh_plan* p, const Switches& sw, uint32_t passable_below);

}  // namespace plan
}  // namespace mh
