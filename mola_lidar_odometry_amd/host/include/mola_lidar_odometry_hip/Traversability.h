// Traversability.h -- a 2.5-D elevation map with a traversability cost from the key-frames of a recorded session (DESIGN.md
// section 0 row g14).  The occupancy grid of row g12 cuts a fixed height band out of the world; outdoors the ground itself rises
// and falls through any band.  This product says what the ground height is, and where a vehicle of a given height and step
// capability can drive.
//
//   once   [host]    the frames and layers of one target map of the header (session_map_frames)
//   once   [device]  ONE mh_elev_bounds_frames + margin = the window
//   once   [device]  ONE mh_elev_add_frames (the ground), ONE mh_elev_mark_frames (obstacles over the finished ground)
//   once   [device]  mh_elev_relief(1) and mh_elev_relief(slope_radius_cells); the download
//   once   [host]    the cost rule, in integers; the files
//
// THE RULE.  Cells, heights, passes and the relief are include/molahip_elevation.h's, word for word.  What the host adds:
//   1. Integers, derived once in fp64:  clearance_q = floor(vehicle_height / z_quantum),  step_q = floor(max_step / z_quantum),
//      rise_q = floor(tan(max_slope_deg * pi / 180) * slope_radius_cells * resolution / z_quantum).
//   2. Window.  x0 = lo_x - margin_cells, nx = hi_x - lo_x + 1 + 2 * margin_cells, and the same in y, lo / hi from the bounds call.
//   3. Cost, per cell, with relief1 = relief(1, min_points_per_cell) and reliefR = relief(slope_radius_cells, min_points_per_cell):
//        UNKNOWN (255)  where count < min_points_per_cell;
//        LETHAL  (254)  else where obstacle_count >= min_obstacle_points, or relief1 > step_q, or reliefR > rise_q;
//        otherwise      max(252 * relief1 / (step_q + 1), 252 * reliefR / (rise_q + 1)), integer division: 0 .. 251.
//      Height [m] = (float)(ground * z_quantum) with the product in fp64; NaN where the cell is unknown.
//   4. Files.  prefix.pgm + prefix.yaml: the trinary pair of OccupancyGrid.h (lethal = occupied, known and not lethal = free), read
//      back by read_occupancy_grid.  prefix_cost.pgm: binary P5, the cost bytes, row 0 at the top = the LARGEST y.
//      prefix_height.f32: little-endian float32, ny * nx, row 0 = the SMALLEST y.  prefix.yaml carries four more lines behind the
//      map-server keys:  cost_image: <name>_cost.pgm\nheight_file: <name>_height.f32\nz_quantum: Q\nheight_row_order: bottom_up\n
//
// Not built: ray-traced free space; sensor origins other than the vehicle pose; a ground estimate that is robust against returns
// from below the ground (the ground of a cell is its lowest point); incremental use while driving.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "molahip_elevation.h"
#include "molahip_host/keyframe_file.h"
#include "mp2p_icp_hip/mp2p_icp_hip.h"

namespace mola_hip {

using mp2p_icp_hip::Config;
using mp2p_icp_hip::DeviceContext;

// the optional top-level traversability: block of the pipeline file (this implementation's own key); an absent block gives the
// defaults.  An unknown key, or a value outside its range: std::runtime_error naming traversability: and the key.
struct TraversabilityOptions {
  double resolution = 0.20;             // cell size [m] > 0
  double z_quantum = 0.01;              // height quantum [m] > 0
  double max_range = 0.0;               // point range limit [m]; 0 = none
  double vehicle_height = 2.0;          // heights above this over the ground are overhead [m] > 0
  double max_step = 0.15;               // largest passable step [m] >= 0
  uint32_t slope_radius_cells = 2;      // radius of the slope window, 1 .. 4
  double max_slope_deg = 20.0;          // largest passable slope, inside (0, 90)
  uint32_t min_points_per_cell = 2;     // points a cell needs to be known, >= 1
  uint32_t min_obstacle_points = 2;     // obstacle points that make a cell lethal, >= 1
  std::string target_map;               // which map of the header the layers are taken from; empty = the first
  uint32_t margin_cells = 2;            // window margin around the bounds
  static TraversabilityOptions FromConfig(const Config& pipeline);
  void validate() const;
  int32_t clearanceQ() const;
  int32_t stepQ() const;
  int32_t riseQ() const;
};

constexpr uint8_t kCostUnknown = 255, kCostLethal = 254;

struct TraversabilityMap {
  int32_t x0 = 0, y0 = 0;  // cell index of column 0 / row 0
  uint32_t nx = 0, ny = 0;
  double resolution = 0, z_quantum = 0;
  int32_t clearance_q = 0, step_q = 0, rise_q = 0;
  uint32_t min_points_per_cell = 1, min_obstacle_points = 1;
  // ny * nx, y outer (the planes and reliefs are empty for a map read back from files)
  std::vector<int32_t> ground, top, relief1, reliefR;
  std::vector<uint32_t> count, obstacle_count;
  std::vector<uint8_t> cost;   // kCostUnknown, kCostLethal or 0 .. 251
  std::vector<float> height;   // [m], NaN where unknown
  uint64_t cells_lethal = 0, cells_free = 0, cells_unknown = 0;
  uint64_t frames = 0, points = 0, points_counted = 0, points_left_out = 0, points_outside_window = 0;
  double seconds_bounds = 0, seconds_add = 0, seconds_mark = 0, seconds_relief = 0;
};

// ---- host rules (testable without a device)
// rule 3: fills m.cost, m.height and the three counts from the planes, the two reliefs and the integers of m
void traversability_classify(TraversabilityMap& m);
// rule 4 (needs cost, height, the window, resolution and z_quantum); read_traversability_map gives those back, and the counts
void write_traversability_map(const TraversabilityMap& m, const std::string& prefix);
TraversabilityMap read_traversability_map(const std::string& prefix);

// ---- the whole thing.  max_points_per_pass: the point passes' (0 = the library's).
TraversabilityMap build_traversability_map(const molahip_host::KeyFrameSet& set, const TraversabilityOptions& opt,
                                           std::shared_ptr<DeviceContext> ctx = nullptr, uint64_t max_points_per_pass = 0);

}  // namespace mola_hip
