// Replan.h -- routes that follow a costmap while its base plane changes under the vehicle.  RoutePlan.h
// builds a costmap, a field and a route once; this product keeps the three alive: a rectangle of the base changes (a lorry parks, a
// gate closes, a door opens), the costmap is inflated again, and the cost-to-go field is REPAIRED round the change
// (include/molahip_replan.h) instead of being computed from nothing.  A moving vehicle costs one trace per question: the field is the
// cost-to-go to the goal from everywhere.
//
//   once       [host]    the price table, the inflation table, the goal's cell
//   once       [device]  ONE mh_nav_set_base + mh_nav_inflate, ONE mh_plan_set_cost_from_nav, ONE mh_plan_field
//   per update [device]  ONE mh_nav_set_base + mh_nav_inflate (the whole window), ONE mh_replan_update_cost_from_nav (the grown rectangle)
//   per route  [device]  ONE mh_plan_trace
//
// THE RULE.  Field, trace and update are include/molahip_plan.h's and include/molahip_replan.h's, word for word; price table, cells,
// route and files are RoutePlan.h's rules 1 to 4.  What this adds:
//   5. The grown rectangle.  update(col0, row0, w, h, bytes) writes the rectangle into the base plane.  A base change moves d2, and
//      with it the cost, only within max_cells cells of it (NavCostmap.h rule 2: the table ends at R = max_cells, a cell further than
//      that from every changed cell sees the same nearest obstacles within R as before).  So the cost plane is handed to the plan as
//      the rectangle [col0 - max_cells, col0 + w + max_cells) x [row0 - max_cells, row0 + h + max_cells), clipped to the window.
//   6. The goal.  Its cell is fixed when the planner is made; it must lie inside the window (a planner whose goal is outside is
//      refused).  A goal cell that an update closes gives status goal_blocked until an update opens it again.
//   7. routeFrom(x, y): RoutePlan.h's rule 3 on the current costmap -- start_outside, start_blocked, goal_blocked, unreachable,
//      truncated, found.  The RoutePlan carries no field plane (field is empty; cells_with_field, sweeps and tile_runs are those of the
//      plan's last field or update).
//   8. The events text.  One event per line; '#' begins a comment; blank lines are skipped; words are separated by blanks or tabs.
//        block X0 Y0 X1 Y1   the base of the rectangle with these two corners [m] becomes 254 (lethal)
//        clear X0 Y0 X1 Y1   ... becomes 0
//        at X Y              a route from this point [m] is asked for
//      Numbers are decimal, read whole by strtod, finite.  Anything else -- an unknown verb (verbs are lower case), a wrong number of
//      numbers, a word that is no number -- is refused with "events: line N: ...", N counting from 1, before any device work.
//   9. A metre rectangle becomes cells by route_cell's floor rule (NavCostmap.h rule 3) on both corners, per axis; the corners may come
//      in either order.  The cell range is inclusive and clipped to the window.  A rectangle with no cell left is counted
//      (ReplanRun::rects_outside) and is not an error; a corner without a cell index (the scaled value reaches 1e6) is refused naming
//      the line.
//
// NOT BUILT: a change of goal or prices without a new planner; a moving window; several rectangles per update; any-angle or kinematic
// routes; a planner under --devices (one device per planner).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "mola_lidar_odometry_hip/RoutePlan.h"
#include "molahip_replan.h"

namespace mola_hip {

struct CellRect {
  bool empty = true;  // no cell of the window
  uint32_t col0 = 0, row0 = 0, w = 0, h = 0;
};

struct ReplanEvent {
  enum Verb { kBlock, kClear, kAt } verb = kAt;
  double v[4] = {0, 0, 0, 0};  // X0 Y0 X1 Y1, or X Y
  uint32_t line = 0;
  const char* verbName() const { return verb == kBlock ? "block" : verb == kClear ? "clear" : "at"; }
};

// ---- host rules (testable without a device)
std::vector<ReplanEvent> parse_replan_events(const std::string& text);                               // rule 8
std::vector<ReplanEvent> read_replan_events(const std::string& path);                                // ... from a file
CellRect replan_metre_rect(const NavCostmap& window, double xa, double ya, double xb, double yb);    // rule 9 (reads the window and the resolution)
CellRect replan_grown_rect(const CellRect& r, uint32_t max_cells, uint32_t nx, uint32_t ny);         // rule 5

// what one update did (mh_replan_info's figures) and what it took
struct ReplanUpdate {
  CellRect rect, grown;
  mh_replan_info info{};
  double seconds_inflate = 0, seconds_update = 0;
};

class RoutePlanner {
 public:
  // `base`, `poses` and `copt` as build_costmap; the goal is ropt's goal_x / goal_y (needed), its start is not used
  RoutePlanner(CostmapBase base, std::vector<Pose12> poses, const NavCostmapOptions& copt, const RouteOptions& ropt,
               std::shared_ptr<DeviceContext> ctx = nullptr);
  ~RoutePlanner();
  RoutePlanner(const RoutePlanner&) = delete;
  RoutePlanner& operator=(const RoutePlanner&) = delete;
  // rule 5.  `bytes`: h * w base bytes, y outer.  Throws when the rectangle is empty or leaves the window.
  ReplanUpdate update(uint32_t col0, uint32_t row0, uint32_t w, uint32_t h, const uint8_t* bytes);
  ReplanUpdate fill(const CellRect& r, uint8_t byte);  // the whole rectangle one byte
  RoutePlan routeFrom(double x, double y);             // rule 7
  // the current costmap (d2, cost, the reach plane of the first build; the counts of costmap_summarise on the current planes)
  const NavCostmap& costmap();
  const CostmapBase& base() const { return base_; }
  uint32_t maxCells() const { return max_cells_; }
  mh_plan_info planInfo() const;

 private:
  void inflate();
  CostmapBase base_;
  std::vector<Pose12> poses_;
  NavCostmapOptions copt_;
  RouteOptions ropt_;
  std::shared_ptr<DeviceContext> ctx_;
  std::vector<uint8_t> table_;
  std::vector<uint16_t> price_;
  uint32_t max_cells_ = 0;
  int32_t goal_col_ = -1, goal_row_ = -1;
  mh_nav* nav_ = nullptr;
  mh_plan* plan_ = nullptr;
  NavCostmap map_;
  bool map_current_ = false;
};

// ---- the whole thing: the source map and the base as build_costmap_from_keyframes, then the events in order
struct ReplanEventResult {
  ReplanEvent event;
  ReplanUpdate update;  // block / clear
  int64_t route = -1;   // at: the index into ReplanRun::routes
};
struct ReplanRun {
  NavCostmap costmap;  // after the last event
  std::vector<ReplanEventResult> events;
  std::vector<RoutePlan> routes;          // one per `at`, in order
  std::vector<NavCostmap> route_costmaps;  // the costmap each route was traced on (cost and d2 as they were then)
  uint64_t rects_outside = 0;
};
ReplanRun replan_route_from_keyframes(const molahip_host::KeyFrameSet& set, const Config& pipeline, const std::vector<ReplanEvent>& events,
                                      std::shared_ptr<DeviceContext> ctx = nullptr);
// write_route for every route of the run: prefix_route_K.txt and prefix_route_K.pgm for the K-th `at`, from 0
void write_replan_routes(const ReplanRun& run, const std::string& prefix);
// the one-line summary of an event, as JSON (the command line prints one per event)
std::string replan_event_summary(const ReplanRun& run, size_t k);

}  // namespace mola_hip
