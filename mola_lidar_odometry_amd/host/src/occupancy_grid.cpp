// occupancy_grid.cpp -- see mola_lidar_odometry_hip/OccupancyGrid.h.  Host logic only: the device is reached through the three
// CVoxelMap methods over include/molahip_occgrid.h.
#include "mola_lidar_odometry_hip/OccupancyGrid.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "config_block.h"
#include "map_files.h"
#include "mola_lidar_odometry_hip/LidarOdometry.h"

namespace mola_hip {

namespace {

const char* const kBlock = "occupancy_grid";

[[noreturn]] void bad(const std::string& key, const std::string& what) { bad_option(kBlock, key, what); }

bool in01(double p) { return p > 0.0 && p < 1.0; }

uint8_t trinary_byte(uint8_t cell) { return (int8_t)cell == kGridOccupied ? 0 : (int8_t)cell == kGridFree ? 254 : 205; }

}  // namespace

// ================================================================== options
OccupancyGridOptions OccupancyGridOptions::FromConfig(const Config& cfg) {
  OccupancyGridOptions o;
  if (cfg.has(kBlock) && !cfg[kBlock].isNull()) {
    const ConfigBlock c(cfg[kBlock], kBlock);
    c.knownKeys({"resolution", "prob_hit", "prob_miss", "clamp_min", "clamp_max", "occupied_threshold", "ray_trace_free_space", "max_range",
                 "decimation", "update_rule", "target_map", "z_min", "z_max", "margin_cells"});
    c.number("resolution", o.resolution);
    c.number("prob_hit", o.prob_hit); c.number("prob_miss", o.prob_miss);
    c.number("clamp_min", o.clamp_min); c.number("clamp_max", o.clamp_max);
    c.number("occupied_threshold", o.occupied_threshold);
    c.boolean("ray_trace_free_space", o.ray_trace_free_space);
    c.number("max_range", o.max_range);
    c.count("decimation", o.decimation);
    c.text("update_rule", o.update_rule);
    c.text("target_map", o.target_map);
    c.number("z_min", o.z_min); c.number("z_max", o.z_max);
    c.count("margin_cells", o.margin_cells);
  }
  o.validate();
  return o;
}

void OccupancyGridOptions::validate() const {
  if (!(resolution > 0.0) || !std::isfinite(resolution)) bad("resolution", "must be finite and > 0");
  if (!in01(prob_hit)) bad("prob_hit", "must lie inside (0, 1)");
  if (!in01(prob_miss)) bad("prob_miss", "must lie inside (0, 1)");
  if (!in01(clamp_min)) bad("clamp_min", "must lie inside (0, 1)");
  if (!in01(clamp_max) || !(clamp_min < clamp_max)) bad("clamp_max", "must lie inside (clamp_min, 1)");
  if (!in01(occupied_threshold)) bad("occupied_threshold", "must lie inside (0, 1)");
  if (!(max_range >= 0.0) || !std::isfinite(max_range)) bad("max_range", "must be finite and >= 0");
  if (decimation < 1) bad("decimation", "must be an integer >= 1");
  if (update_rule != "counted" && update_rule != "once") bad("update_rule", "must be counted or once");
  if (!std::isfinite(z_min)) bad("z_min", "must be finite");
  if (!std::isfinite(z_max) || !(z_min <= z_max)) bad("z_max", "must be finite and >= z_min");
  if (margin_cells > 65536) bad("margin_cells", "must be <= 65536");
  for (double z : {z_min, z_max})
    if (!(std::fabs(z * (double)(1.0f / (float)resolution)) < 1.0e6)) bad(z == z_min ? "z_min" : "z_max", "lies outside the key range of the map");
}

mh_occmap_params OccupancyGridOptions::deviceParams() const {
  mh_occmap_params p = mp2p_icp_hip::CVoxelMap::defaultParams((float)resolution);
  p.prob_hit = (float)prob_hit; p.prob_miss = (float)prob_miss;
  p.clamp_min = (float)clamp_min; p.clamp_max = (float)clamp_max;
  p.occupied_threshold = (float)occupied_threshold;
  p.ray_trace_free_space = ray_trace_free_space ? 1u : 0u;
  p.decimation = decimation;
  p.max_range = (float)max_range;
  p.update_rule = update_rule == "once" ? MH_OCC_ONCE : MH_OCC_COUNTED;
  p.index_mode = MH_INDEX_FLOOR;  // (rule 1 is the floor rule)
  return p;
}

// ================================================================== host rules
int32_t occupancy_grid_z_index(double z, double resolution) { return (int32_t)std::floor(z * (double)(1.0f / (float)resolution)); }

void occupancy_grid_classify(OccupancyGrid& g) {
  const size_t n = (size_t)g.nx * g.ny;
  if (g.max_logodds.size() != n) throw std::runtime_error("occupancy_grid_classify: max_logodds needs ny * nx entries");
  g.cells.resize(n);
  g.cells_occupied = g.cells_free = g.cells_unknown = 0;
  for (size_t i = 0; i < n; i++) {
    const int32_t m = g.max_logodds[i];
    if (m == MH_OCCGRID_NONE) { g.cells[i] = kGridUnknown; g.cells_unknown++; }
    else if (m >= g.l_occ) { g.cells[i] = kGridOccupied; g.cells_occupied++; }
    else { g.cells[i] = kGridFree; g.cells_free++; }
  }
}

void write_occupancy_grid(const OccupancyGrid& g, const std::string& prefix) {
  const size_t n = (size_t)g.nx * g.ny;
  if (g.cells.size() != n || n == 0) throw std::runtime_error("write_occupancy_grid: the grid holds no cells");
  write_file("write_occupancy_grid", prefix + ".pgm", pgm_bytes((const uint8_t*)g.cells.data(), g.nx, g.ny, trinary_byte), std::ios::trunc);
  write_file("write_occupancy_grid", prefix + ".yaml",
             "image: " + base_name(prefix) + ".pgm\nresolution: " + g9(g.resolution) + "\norigin: [" + g9((double)g.x0 * g.resolution) + ", " +
                 g9((double)g.y0 * g.resolution) + ", 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n",
             std::ios::trunc);
}

OccupancyGrid read_occupancy_grid(const std::string& prefix) {
  OccupancyGrid g;
  const std::string yaml = slurp("read_occupancy_grid", prefix + ".yaml"), path = prefix + ".pgm";
  std::string res, origin;
  double ox = 0, oy = 0;
  if (!yaml_line(yaml, "resolution:", res) || !yaml_line(yaml, "origin:", origin) || sscanf(origin.c_str(), " [%lf , %lf", &ox, &oy) != 2 ||
      !((g.resolution = strtod(res.c_str(), nullptr)) > 0.0))
    throw std::runtime_error("read_occupancy_grid: '" + prefix + ".yaml' lacks resolution or origin");
  g.x0 = (int32_t)std::llround(ox / g.resolution);
  g.y0 = (int32_t)std::llround(oy / g.resolution);
  std::vector<uint8_t> bytes;
  if (!pgm_plane(slurp("read_occupancy_grid", path), 0, 0, g.nx, g.ny, bytes))
    throw std::runtime_error("read_occupancy_grid: '" + path + "' is not a binary PGM written by write_occupancy_grid");
  g.cells.resize(bytes.size());
  for (size_t i = 0; i < bytes.size(); i++) {
    const uint8_t v = bytes[i];
    if (v == 0) { g.cells[i] = kGridOccupied; g.cells_occupied++; }
    else if (v == 254) { g.cells[i] = kGridFree; g.cells_free++; }
    else if (v == 205) { g.cells[i] = kGridUnknown; g.cells_unknown++; }
    else throw std::runtime_error("read_occupancy_grid: '" + path + "' holds a byte that is neither 0, 254 nor 205");
  }
  return g;
}

// ================================================================== the whole thing
OccupancyGrid build_occupancy_grid(const molahip_host::KeyFrameSet& set, const OccupancyGridOptions& opt, std::shared_ptr<DeviceContext> ctx,
                                   uint64_t max_points_per_pass) {
  opt.validate();
  const size_t map_index = target_map_index(set, opt.target_map, "build_occupancy_grid", kBlock);
  const std::vector<mp2p_icp_hip::PosedFrame> frames = session_map_frames(set, map_index);
  OccupancyGrid g;
  g.resolution = opt.resolution;
  g.frames = frames.size();
  for (const auto& f : frames) g.points += f.n;
  if (!g.points)
    throw std::runtime_error("build_occupancy_grid: the key-frames hold no points for target map '" + set.maps[map_index].name + "'");
  if (!ctx) ctx = DeviceContext::Default();
  using clock = std::chrono::steady_clock;
  mp2p_icp_hip::CVoxelMap map(opt.deviceParams(), ctx);
  auto t0 = clock::now();
  map.insertPointCloudFrames(frames, max_points_per_pass);
  g.seconds_insert = std::chrono::duration<double>(clock::now() - t0).count();
  const mh_occmap_info info = map.occInfo();
  g.l_occ = info.l_occ;
  g.map_cells = info.n_cells;
  int32_t lo[3], hi[3];
  if (!map.indexBounds(lo, hi))
    throw std::runtime_error("build_occupancy_grid: no point of the key-frames fell inside max_range and the key range: the map is empty");
  const int64_t m = opt.margin_cells;
  const int64_t nx = (int64_t)hi[0] - lo[0] + 1 + 2 * m, ny = (int64_t)hi[1] - lo[1] + 1 + 2 * m;
  if (nx * ny > (int64_t)1 << 28) throw std::runtime_error("build_occupancy_grid: the grid would exceed 2^28 cells: raise occupancy_grid: resolution");
  g.x0 = (int32_t)(lo[0] - m);
  g.y0 = (int32_t)(lo[1] - m);
  g.nx = (uint32_t)nx;
  g.ny = (uint32_t)ny;
  g.z_lo = occupancy_grid_z_index(opt.z_min, opt.resolution);
  g.z_hi = occupancy_grid_z_index(opt.z_max, opt.resolution);
  mh_occgrid_window w{};
  w.x0 = g.x0; w.y0 = g.y0; w.nx = g.nx; w.ny = g.ny; w.z_lo = g.z_lo; w.z_hi = g.z_hi;
  t0 = clock::now();
  g.max_logodds = map.projectGrid(w);
  g.seconds_project = std::chrono::duration<double>(clock::now() - t0).count();
  occupancy_grid_classify(g);
  return g;
}

}  // namespace mola_hip
