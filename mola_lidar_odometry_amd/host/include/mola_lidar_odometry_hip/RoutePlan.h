// RoutePlan.h -- a route over an inflated costmap: the cost-to-go field to a goal and the route traced down it from a start
// (DESIGN.md section 0 row g16).  The costmap (g15) says where a vehicle of a given radius may stand; this product says how it gets
// from A to B over those cells, and what that costs.
//
//   once   [host]    the price table; the start's and the goal's cells
//   once   [device]  ONE mh_plan_set_cost, ONE mh_plan_field from the goal, ONE mh_plan_trace from the start, the download
//                    (include/molahip_plan.h)
//   once   [host]    the route in metres, its summary, the files
//
// THE RULE.  Field and trace are include/molahip_plan.h's, word for word.  What the host adds:
//   1. Price table, in fp64.  price[c] = neutral_price + floor(cost_factor * c) for c = 0 .. 252; passable_below is
//      kCostmapPassableBelow (253).  A table with an entry above 65535 is refused, and so is one that fails the header's wrap-around
//      bound for the costmap's window, with a message that names the largest number of cells the prices admit.
//   2. Cells.  The start's and the goal's cell by the fp32 floor rule of costmap_seeds (NavCostmap.h rule 3), word for word; a point
//      without a cell counts as outside the window.  From key-frames (plan_route_from_keyframes) the metre keys, when present, win;
//      otherwise the translation of key-frame start_keyframe / goal_keyframe is taken, -1 naming the last one.
//   3. Route.  status: start_outside, start_blocked (the start's cost is >= 253), goal_outside, goal_blocked, in this order and
//      before a device is asked for; then unreachable (the start's field is MH_PLAN_UNREACHED), truncated (the route has more than
//      max_route_cells cells: the first max_route_cells are kept) or found.
//      The cells go to metres at cell centres: x = (x0 + column + 0.5) * resolution, y = (y0 + row + 0.5) * resolution.
//      length_m = the fp64 sum, in route order, of resolution per orthogonal step and resolution * sqrt(2.0) per diagonal one.
//      cost_to_go = field[start] (MH_PLAN_UNREACHED when no field was computed or the start is not joined to the goal).
//      max_cost = the largest cost byte over the route's cells (0 for an empty route).
//      min_clearance_m = the minimum of sqrt(d2) * resolution over the route's cells with d2 != MH_NAV_FAR; -1 when there is none,
//      or when the costmap has no d2 (one read back from files).
//   4. Files.  prefix_route.txt: one "x y" line per cell, both as %.9g.  prefix_route.pgm: the trinary image of write_costmap
//      (occupied 0 where cost is 253 or 254, unknown 205 where 255, free 254 otherwise) with every route cell drawn as 100; row 0 at
//      the top is the largest y.
//
// NOT BUILT: any-angle or kinematic routes; footprints other than a disc; a route under --devices (one device per call).  (Replanning
// while the costmap changes: Replan.h.)
#pragma once
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "mola_lidar_odometry_hip/NavCostmap.h"
#include "molahip_plan.h"

namespace mola_hip {

// the optional top-level route: block of the pipeline file (this implementation's own key); an absent block gives the defaults.
// An unknown key, or a value outside its range: std::runtime_error naming route: and the key.
struct RouteOptions {
  double start_x = std::numeric_limits<double>::quiet_NaN(), start_y = std::numeric_limits<double>::quiet_NaN();  // [m]; NaN: not given
  double goal_x = std::numeric_limits<double>::quiet_NaN(), goal_y = std::numeric_limits<double>::quiet_NaN();
  int64_t start_keyframe = 0, goal_keyframe = -1;  // used when the metre keys are absent; -1: the last key-frame
  uint32_t neutral_price = 4;                      // >= 1
  double cost_factor = 0.08;                       // >= 0
  uint32_t max_route_cells = 1048576;              // >= 1: the trace's cap
  static RouteOptions FromConfig(const Config& pipeline);
  void validate() const;
  bool hasStart() const { return start_x == start_x; }  // (validate() holds x and y together)
  bool hasGoal() const { return goal_x == goal_x; }
};

struct RoutePlan {
  std::string status;
  int32_t start_col = -1, start_row = -1, goal_col = -1, goal_row = -1;  // relative to the window; -1 outside
  std::vector<int32_t> cells;  // (column, row) pairs in route order
  std::vector<double> xy;      // (x, y) pairs [m]
  double length_m = 0;
  uint32_t cost_to_go = MH_PLAN_UNREACHED, max_cost = 0;
  double min_clearance_m = -1.0;
  std::vector<uint32_t> field;  // ny * nx, y outer; empty when the status was decided before the device
  uint32_t sweeps = 0;
  uint64_t tile_runs = 0, cells_with_field = 0;
  double seconds_field = 0, seconds_trace = 0;
};

// ---- host rules (testable without a device)
std::vector<uint16_t> route_price_table(const RouteOptions& opt);  // rule 1: 253 entries
// rule 1's second refusal: throws naming route: when the table fails the wrap-around bound for a window of n_cells cells
void route_check_window(const std::vector<uint16_t>& price, uint64_t n_cells);
// rule 2: false when the point has no cell in the window (col = row = -1)
bool route_cell(const NavCostmap& c, double x, double y, int32_t& col, int32_t& row);
// rule 3: xy, length_m, max_cost and min_clearance_m from r.cells
void route_summarise(RoutePlan& r, const NavCostmap& c);
// rule 4; `stem` stands for "_route" in the two file names (Replan.h writes prefix_route_K.txt / .pgm with it)
void write_route(const RoutePlan& r, const NavCostmap& c, const std::string& prefix, const std::string& stem = "_route");

// ---- the whole thing.  plan_route needs the four metre keys.
RoutePlan plan_route(const NavCostmap& c, const RouteOptions& opt, std::shared_ptr<DeviceContext> ctx = nullptr);
struct RouteFromKeyframes {
  NavCostmap costmap;
  RoutePlan route;
};
RouteFromKeyframes plan_route_from_keyframes(const molahip_host::KeyFrameSet& set, const Config& pipeline,
                                             std::shared_ptr<DeviceContext> ctx = nullptr);

}  // namespace mola_hip
