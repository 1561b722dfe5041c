// OccupancyGrid.h -- a navigation occupancy grid from the key-frames of a recorded session.  Every
// other product of a key-frame file is points; this one says where the vehicle may drive: occupied, free and unknown cells.
//
//   once   [host]    the frames and layers of one target map of the header (session_map_frames)
//   once   [device]  ONE fresh CVoxelMap, ONE insertPointCloudFrames (mh_occmap_insert_frames: every key-frame ray-traced from its pose)
//   once   [device]  indexBounds() + margin = the window; ONE projectGrid of the height band (mh_occmap_project_grid)
//   once   [host]    the trinary rule; the PGM / YAML pair that map servers load
//
// THE RULE.  Insertion, bounds and projection are include/molahip_occgrid.h's, word for word.  What the host adds:
//   1. Height band.  z_min, z_max [m, world frame] become inclusive cell indices by the map's floor rule in fp64:
//      index(z) = floor(z * (double)(1.0f / (float)resolution)).
//   2. Window.  x0 = lo_x - margin_cells, nx = hi_x - lo_x + 1 + 2 * margin_cells, and the same in y, with lo / hi the index bounds
//      over ALL stored cells (whatever their height).
//   3. Trinary rule, per grid cell with m = the projected maximum:  UNKNOWN (-1) where m == MH_OCCGRID_NONE;  OCCUPIED (100) where
//      m >= l_occ (mh_occmap_info);  FREE (0) otherwise.
//   4. Files.  prefix.pgm: binary P5, "P5\n<nx> <ny>\n255\n", then ny rows of nx bytes, row 0 at the top = the LARGEST y; 0 occupied,
//      254 free, 205 unknown.  prefix.yaml: the map-server keys, one per line, numbers as %.9g:
//        image: <file name of the pgm>\nresolution: R\norigin: [X, Y, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n
//      with X = x0 * R, Y = y0 * R in fp64 (the world position of the lower-left corner of the lower-left cell).
//
// A key-frame file of ANY plan is accepted, a CVoxelMap plan included: the frames carry layers and poses whatever the target class
// (this is how a lidar2d session gets its grid).  Not built: sensor origins other than the vehicle pose (rays start at the cell of
// the key-frame's translation); far removal; a snapshot of the occupancy map (still refused); 3-D grid export.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "molahip_host/keyframe_file.h"
#include "molahip_occgrid.h"
#include "mp2p_icp_hip/mp2p_icp_hip.h"

namespace mola_hip {

using mp2p_icp_hip::Config;
using mp2p_icp_hip::DeviceContext;

// the optional top-level occupancy_grid: block of the pipeline file (this implementation's own key); an absent block gives the
// defaults.  An unknown key, or a value outside its range: std::runtime_error naming occupancy_grid: and the key.
struct OccupancyGridOptions {
  double resolution = 0.05;                     // [m] > 0
  double prob_hit = 0.70, prob_miss = 0.30;     // lidar2d.yaml's values
  double clamp_min = 0.05, clamp_max = 0.95;
  double occupied_threshold = 0.60;
  bool ray_trace_free_space = true;
  double max_range = 0.0;                       // [m]; 0 = no limit
  uint32_t decimation = 1;                      // >= 1
  std::string update_rule = "counted";          // "counted" or "once" (MH_OCC_*)
  std::string target_map;                       // which map of the header the layers are taken from; empty = the first
  double z_min = -0.10, z_max = 1.50;           // [m], world frame; z_min <= z_max
  uint32_t margin_cells = 2;
  static OccupancyGridOptions FromConfig(const Config& pipeline);
  void validate() const;
  mh_occmap_params deviceParams() const;
};

constexpr int8_t kGridFree = 0, kGridOccupied = 100, kGridUnknown = -1;

struct OccupancyGrid {
  int32_t x0 = 0, y0 = 0;   // cell index of column 0 / row 0
  uint32_t nx = 0, ny = 0;
  double resolution = 0;
  int32_t z_lo = 0, z_hi = 0, l_occ = 0;
  std::vector<int32_t> max_logodds;  // ny * nx, y outer (empty for a grid read back from files)
  std::vector<int8_t> cells;         // ny * nx, y outer: kGridFree / kGridOccupied / kGridUnknown
  uint64_t cells_occupied = 0, cells_free = 0, cells_unknown = 0;
  uint64_t frames = 0, points = 0, map_cells = 0;  // what went in; the stored cells of the occupancy map
  double seconds_insert = 0, seconds_project = 0;
};

// ---- host rules (testable without a device)
int32_t occupancy_grid_z_index(double z, double resolution);  // rule 1
// rule 3: fills g.cells and the three counts from g.max_logodds and g.l_occ
void occupancy_grid_classify(OccupancyGrid& g);
// rule 4; read_occupancy_grid gives back x0, y0, nx, ny, the resolution, the cells and the counts
void write_occupancy_grid(const OccupancyGrid& g, const std::string& prefix);
OccupancyGrid read_occupancy_grid(const std::string& prefix);

// ---- the whole thing.  max_points_per_pass: mh_occmap_insert_frames' (0 = the library's).
OccupancyGrid build_occupancy_grid(const molahip_host::KeyFrameSet& set, const OccupancyGridOptions& opt,
                                   std::shared_ptr<DeviceContext> ctx = nullptr, uint64_t max_points_per_pass = 0);

}  // namespace mola_hip
