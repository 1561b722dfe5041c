// NavCostmap.h -- an inflated costmap, the clearance and the reachable region from a session's maps (DESIGN.md section 0 row
// g15).  The occupancy grid (g12) and the traversability map (g14) judge a cell as if the vehicle were a point.  This product says
// where a vehicle of a given radius can stand, and which of those cells it can get to from where it drove.
//
//   once   [host]    the base plane from the source map; the inflation table; the seeds from the key-frame poses
//   once   [device]  ONE mh_nav_set_base, ONE mh_nav_inflate, ONE mh_nav_reach, the download (include/molahip_nav.h)
//   once   [host]    counts, the trajectory's clearance, the files
//
// THE RULE.  Distance, cost and reach are include/molahip_nav.h's, word for word.  What the host adds:
//   1. Base plane.  From a TraversabilityMap: its cost bytes as they are.  From an OccupancyGrid: occupied -> 254, unknown -> 255,
//      free -> 0.  Window and resolution are the source map's.
//   2. Table, in fp64.  R = ceil(inflation_radius / resolution), refused above 255.  table[0] = 0; for d2 = 1 .. R * R with
//      d = sqrt((double)d2) * resolution:  253 when d <= inscribed_radius;  otherwise
//      floor(252 * exp(-cost_scaling * (d - inscribed_radius))) when d <= inflation_radius;  otherwise 0.
//   3. Seeds.  The cell of a key-frame's translation t by the floor rule both source maps use for x and y:
//      (int32) floorf((float)t * (1.0f / (float)resolution)) per axis in fp32, un-fused, less the window's x0 / y0; a translation
//      that is not finite or whose scaled value reaches 1e6 in magnitude has no cell (it counts as outside the window).
//      reach_from: keyframes = all of them, first = the first key-frame only, none = no seed (reach is all zero).
//      passable_below is 253: a cell is passable when the vehicle's centre may stand there.
//   4. Counts, over the window:  unknown (cost 255), lethal (254), inscribed (253);  of the cells below 253: inflated where
//      d2 != MH_NAV_FAR, free where d2 == MH_NAV_FAR;  reached (reach == 1);  unreachable_free = cells below 253 with reach == 0.
//      Per key-frame: d2, cost and reached of its cell (MH_NAV_FAR, 255, 0 for a key-frame without a cell in the window).
//      keyframes_blocked = key-frames whose cost is >= 253: the recorded drive passes through cells this radius forbids, so the
//      chosen radius is larger than the vehicle that drove it.  trajectory_min_clearance_m = the minimum over the key-frames with
//      d2 != MH_NAV_FAR of sqrt(d2) * resolution; -1 when no key-frame has an obstacle within the inflation radius.
//   5. Files.  prefix.pgm + prefix.yaml: the trinary pair of OccupancyGrid.h (occupied where cost is 253 or 254, unknown where 255,
//      free otherwise), read back by read_occupancy_grid.  prefix_cost.pgm: binary P5, the cost bytes, row 0 at the top = the LARGEST
//      y (the traversability map's convention).  prefix_reach.pgm: the same shape, 255 reached and 0 not.  prefix.yaml carries four
//      more lines behind the map-server keys:
//        cost_image: <name>_cost.pgm\nreach_image: <name>_reach.pgm\ninscribed_radius: A\ninflation_radius: B\n   (numbers as %.9g)
//      read_costmap gives back the window, the resolution, cost, reach, the two radii and the counts that need no d2.
//
// NOT BUILT: footprints other than a disc; 8-connectivity; a distance beyond 255 cells; an incremental inflation (Replan.h inflates
// the whole window again after a change of the base and repairs only the route field); a costmap under --devices (one device per
// call).  (Routes over the costmap: RoutePlan.h; routes while the base changes: Replan.h.)
#pragma once
#include <array>
#include <memory>
#include <string>
#include <vector>

#include "mola_lidar_odometry_hip/OccupancyGrid.h"
#include "mola_lidar_odometry_hip/Traversability.h"
#include "molahip_host/keyframe_file.h"
#include "molahip_nav.h"
#include "mp2p_icp_hip/mp2p_icp_hip.h"

namespace mola_hip {

// the optional top-level costmap: block of the pipeline file (this implementation's own key); an absent block gives the defaults.
// An unknown key, or a value outside its range: std::runtime_error naming costmap: and the key.
struct NavCostmapOptions {
  std::string source = "traversability";   // "traversability" or "occupancy_grid": which builder build_costmap_from_keyframes runs
  double inscribed_radius = 0.5;           // [m] >= 0: the vehicle's radius
  double inflation_radius = 1.5;           // [m] >= inscribed_radius; ceil(inflation_radius / resolution) <= 255
  double cost_scaling = 3.0;               // [1/m] > 0
  bool unknown_is_obstacle = false;
  std::string reach_from = "keyframes";    // "keyframes", "first" or "none"
  static NavCostmapOptions FromConfig(const Config& pipeline);
  void validate() const;
  uint32_t maxCells(double resolution) const;  // rule 2's R; throws naming costmap: inflation_radius when it exceeds 255
};

constexpr uint32_t kCostmapPassableBelow = 253;
using Pose12 = std::array<double, 12>;

struct CostmapBase {
  int32_t x0 = 0, y0 = 0;
  uint32_t nx = 0, ny = 0;
  double resolution = 0;
  std::vector<uint8_t> bytes;  // ny * nx, y outer
};

struct NavCostmap {
  int32_t x0 = 0, y0 = 0;
  uint32_t nx = 0, ny = 0;
  double resolution = 0, inscribed_radius = 0, inflation_radius = 0;
  uint32_t max_cells = 0;
  bool unknown_is_obstacle = false;
  // ny * nx, y outer (d2 is empty for a costmap read back from files)
  std::vector<uint16_t> d2;
  std::vector<uint8_t> cost, reach;
  uint64_t cells_lethal = 0, cells_inscribed = 0, cells_inflated = 0, cells_free = 0, cells_unknown = 0, cells_reached = 0,
           cells_unreachable_free = 0;
  std::vector<uint16_t> keyframe_d2;
  std::vector<uint8_t> keyframe_cost, keyframe_reached;
  double trajectory_min_clearance_m = -1.0;
  uint64_t keyframes_blocked = 0;
  uint64_t seeds = 0, seeds_blocked = 0, seeds_outside = 0;
  uint32_t sweeps = 0;
  double seconds_source = 0, seconds_inflate = 0, seconds_reach = 0;
};

// ---- host rules (testable without a device)
CostmapBase costmap_base(const TraversabilityMap& m);  // rule 1
CostmapBase costmap_base(const OccupancyGrid& g);
std::vector<uint8_t> inflation_table(const NavCostmapOptions& opt, double resolution);  // rule 2: R * R + 1 entries
// rule 3: (column, row) pairs relative to the window, for the key-frames that reach_from selects
std::vector<int32_t> costmap_seeds(const CostmapBase& base, const std::vector<Pose12>& poses, const std::string& reach_from);
// rule 4: the counts and the per-key-frame values from the planes of c (cost and reach of ny * nx entries; d2 of as many, or empty:
// then inflated / free stay 0 and the key-frames' d2 is MH_NAV_FAR)
void costmap_summarise(NavCostmap& c, const std::vector<Pose12>& poses);
// rule 5
void write_costmap(const NavCostmap& c, const std::string& prefix);
NavCostmap read_costmap(const std::string& prefix);

// ---- the whole thing
NavCostmap build_costmap(const CostmapBase& base, const std::vector<Pose12>& poses, const NavCostmapOptions& opt,
                         std::shared_ptr<DeviceContext> ctx = nullptr);
inline NavCostmap build_costmap(const TraversabilityMap& m, const std::vector<Pose12>& poses, const NavCostmapOptions& opt,
                                std::shared_ptr<DeviceContext> ctx = nullptr) {
  return build_costmap(costmap_base(m), poses, opt, std::move(ctx));
}
inline NavCostmap build_costmap(const OccupancyGrid& g, const std::vector<Pose12>& poses, const NavCostmapOptions& opt,
                                std::shared_ptr<DeviceContext> ctx = nullptr) {
  return build_costmap(costmap_base(g), poses, opt, std::move(ctx));
}
// the source map by its own builder and its own block of `pipeline` (traversability: or occupancy_grid:), then the costmap from it
// and the poses of every key-frame of the set
NavCostmap build_costmap_from_keyframes(const molahip_host::KeyFrameSet& set, const Config& pipeline,
                                        std::shared_ptr<DeviceContext> ctx = nullptr);

}  // namespace mola_hip
