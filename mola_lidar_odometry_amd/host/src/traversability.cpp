// traversability.cpp -- see mola_lidar_odometry_hip/Traversability.h.  Host logic only: the device is reached through
// include/molahip_elevation.h.
#include "mola_lidar_odometry_hip/Traversability.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>

#include "config_block.h"
#include "map_files.h"
#include "mola_lidar_odometry_hip/LidarOdometry.h"
#include "mola_lidar_odometry_hip/OccupancyGrid.h"

namespace mola_hip {

namespace {

const char* const kBlock = "traversability";
const double kPi = 3.14159265358979323846;

[[noreturn]] void bad(const std::string& key, const std::string& what) { bad_option(kBlock, key, what); }

const double kQMax = 1073741824.0;  // 2^30: what a height may reach in quanta (molahip_elevation.h, case 3)

}  // namespace

// ================================================================== options
TraversabilityOptions TraversabilityOptions::FromConfig(const Config& cfg) {
  TraversabilityOptions o;
  if (cfg.has(kBlock) && !cfg[kBlock].isNull()) {
    const ConfigBlock c(cfg[kBlock], kBlock);
    c.knownKeys({"resolution", "z_quantum", "max_range", "vehicle_height", "max_step", "slope_radius_cells", "max_slope_deg",
                 "min_points_per_cell", "min_obstacle_points", "target_map", "margin_cells"});
    c.number("resolution", o.resolution);
    c.number("z_quantum", o.z_quantum);
    c.number("max_range", o.max_range);
    c.number("vehicle_height", o.vehicle_height);
    c.number("max_step", o.max_step);
    c.count("slope_radius_cells", o.slope_radius_cells);
    c.number("max_slope_deg", o.max_slope_deg);
    c.count("min_points_per_cell", o.min_points_per_cell);
    c.count("min_obstacle_points", o.min_obstacle_points);
    c.text("target_map", o.target_map);
    c.count("margin_cells", o.margin_cells);
  }
  o.validate();
  return o;
}

void TraversabilityOptions::validate() const {
  if (!(resolution > 0.0) || !std::isfinite(resolution)) bad("resolution", "must be finite and > 0");
  if (!(z_quantum > 0.0) || !std::isfinite(z_quantum)) bad("z_quantum", "must be finite and > 0");
  if (!(max_range >= 0.0) || !std::isfinite(max_range)) bad("max_range", "must be finite and >= 0");
  if (!(vehicle_height > 0.0) || !std::isfinite(vehicle_height) || !(vehicle_height / z_quantum < kQMax))
    bad("vehicle_height", "must be finite, > 0 and below 2^30 height quanta");
  if (!(max_step >= 0.0) || !std::isfinite(max_step) || !(max_step / z_quantum < kQMax)) bad("max_step", "must be finite, >= 0 and below 2^30 height quanta");
  if (slope_radius_cells < 1 || slope_radius_cells > MH_ELEV_MAX_RELIEF_RADIUS) bad("slope_radius_cells", "must be an integer from 1 to 4");
  if (!(max_slope_deg > 0.0) || !(max_slope_deg < 90.0)) bad("max_slope_deg", "must lie inside (0, 90)");
  if (!(std::tan(max_slope_deg * kPi / 180.0) * slope_radius_cells * resolution / z_quantum < kQMax))
    bad("max_slope_deg", "gives a rise of 2^30 height quanta or more over the slope window");
  if (min_points_per_cell < 1) bad("min_points_per_cell", "must be an integer >= 1");
  if (min_obstacle_points < 1) bad("min_obstacle_points", "must be an integer >= 1");
  if (margin_cells > 65536) bad("margin_cells", "must be <= 65536");
}

int32_t TraversabilityOptions::clearanceQ() const { return (int32_t)std::floor(vehicle_height / z_quantum); }
int32_t TraversabilityOptions::stepQ() const { return (int32_t)std::floor(max_step / z_quantum); }
int32_t TraversabilityOptions::riseQ() const {
  return (int32_t)std::floor(std::tan(max_slope_deg * kPi / 180.0) * slope_radius_cells * resolution / z_quantum);
}

// ================================================================== host rules
void traversability_classify(TraversabilityMap& m) {
  const size_t n = (size_t)m.nx * m.ny;
  if (n == 0 || m.ground.size() != n || m.count.size() != n || m.obstacle_count.size() != n || m.relief1.size() != n || m.reliefR.size() != n)
    throw std::runtime_error("traversability_classify: ground, count, obstacle_count, relief1 and reliefR need ny * nx entries each");
  if (m.step_q < 0 || m.rise_q < 0) throw std::runtime_error("traversability_classify: step_q and rise_q must be >= 0");
  m.cost.resize(n);
  m.height.resize(n);
  m.cells_lethal = m.cells_free = m.cells_unknown = 0;
  for (size_t i = 0; i < n; i++) {
    if (m.count[i] < m.min_points_per_cell) {
      m.cost[i] = kCostUnknown;
      m.height[i] = std::numeric_limits<float>::quiet_NaN();
      m.cells_unknown++;
      continue;
    }
    m.height[i] = (float)((double)m.ground[i] * m.z_quantum);
    const int64_t r1 = m.relief1[i], rR = m.reliefR[i];
    if (m.obstacle_count[i] >= m.min_obstacle_points || r1 > m.step_q || rR > m.rise_q) {
      m.cost[i] = kCostLethal;
      m.cells_lethal++;
    } else {  // (r1 <= step_q, rR <= rise_q: both terms are below 252; a relief of a known cell is >= 0)
      m.cost[i] = (uint8_t)std::max(252 * std::max<int64_t>(r1, 0) / ((int64_t)m.step_q + 1), 252 * std::max<int64_t>(rR, 0) / ((int64_t)m.rise_q + 1));
      m.cells_free++;
    }
  }
}

void write_traversability_map(const TraversabilityMap& m, const std::string& prefix) {
  const size_t n = (size_t)m.nx * m.ny;
  if (n == 0 || m.cost.size() != n || m.height.size() != n) throw std::runtime_error("write_traversability_map: the map holds no cells");
  OccupancyGrid g;  // the trinary pair is OccupancyGrid.h's, written by its writer
  g.x0 = m.x0; g.y0 = m.y0; g.nx = m.nx; g.ny = m.ny;
  g.resolution = m.resolution;
  g.cells.resize(n);
  for (size_t i = 0; i < n; i++) g.cells[i] = m.cost[i] == kCostLethal ? kGridOccupied : m.cost[i] == kCostUnknown ? kGridUnknown : kGridFree;
  write_occupancy_grid(g, prefix);
  const char* const who = "write_traversability_map";
  const std::string name = base_name(prefix);
  write_file(who, prefix + ".yaml", "cost_image: " + name + "_cost.pgm\nheight_file: " + name + "_height.f32\nz_quantum: " + g9(m.z_quantum) +
                                        "\nheight_row_order: bottom_up\n", std::ios::app);
  write_file(who, prefix + "_cost.pgm", pgm_bytes(m.cost.data(), m.nx, m.ny), std::ios::trunc);
  std::string f32(n * 4, '\0');
  for (size_t i = 0; i < n; i++) {  // little-endian, whatever the host
    uint32_t u;
    memcpy(&u, &m.height[i], 4);
    for (int b = 0; b < 4; b++) f32[4 * i + b] = (char)((u >> (8 * b)) & 0xFF);
  }
  write_file(who, prefix + "_height.f32", f32, std::ios::trunc);
}

TraversabilityMap read_traversability_map(const std::string& prefix) {
  const OccupancyGrid g = read_occupancy_grid(prefix);  // the window, the resolution, the trinary cells
  TraversabilityMap m;
  m.x0 = g.x0; m.y0 = g.y0; m.nx = g.nx; m.ny = g.ny;
  m.resolution = g.resolution;
  const size_t n = (size_t)m.nx * m.ny;
  const char* const who = "read_traversability_map";
  const std::string yaml = slurp(who, prefix + ".yaml"), dir = dir_of(prefix);
  std::string cost_name, height_name, quantum, order;
  yaml_line(yaml, "cost_image: ", cost_name);
  yaml_line(yaml, "height_file: ", height_name);
  if (yaml_line(yaml, "z_quantum:", quantum)) m.z_quantum = strtod(quantum.c_str(), nullptr);
  yaml_line(yaml, "height_row_order: ", order);
  if (cost_name.empty() || height_name.empty() || !(m.z_quantum > 0.0) || order != "bottom_up")
    throw std::runtime_error("read_traversability_map: '" + prefix + ".yaml' lacks cost_image, height_file, z_quantum or height_row_order: bottom_up");
  {
    const std::string path = dir + cost_name;
    if (!pgm_plane(slurp(who, path), g.nx, g.ny, m.nx, m.ny, m.cost))
      throw std::runtime_error("read_traversability_map: '" + path + "' is not the cost image of '" + prefix + ".pgm'");
    for (size_t i = 0; i < n; i++) {
      const uint8_t c = m.cost[i];
      const int8_t want = c == kCostLethal ? kGridOccupied : c == kCostUnknown ? kGridUnknown : kGridFree;
      if (c == 252 || c == 253 || g.cells[i] != want)
        throw std::runtime_error("read_traversability_map: '" + path + "' disagrees with the trinary image '" + prefix + ".pgm'");
      (c == kCostLethal ? m.cells_lethal : c == kCostUnknown ? m.cells_unknown : m.cells_free)++;
    }
  }
  {
    const std::string path = dir + height_name, s = slurp(who, path);
    if (s.size() != 4 * n) throw std::runtime_error("read_traversability_map: '" + path + "' does not hold ny * nx float32 values");
    m.height.resize(n);
    for (size_t i = 0; i < n; i++) {
      uint32_t u = 0;
      for (int b = 0; b < 4; b++) u |= (uint32_t)(unsigned char)s[4 * i + b] << (8 * b);
      memcpy(&m.height[i], &u, 4);
    }
  }
  return m;
}

// ================================================================== the whole thing
TraversabilityMap build_traversability_map(const molahip_host::KeyFrameSet& set, const TraversabilityOptions& opt,
                                           std::shared_ptr<DeviceContext> ctx, uint64_t max_points_per_pass) {
  using mp2p_icp_hip::check;
  opt.validate();
  const size_t map_index = target_map_index(set, opt.target_map, "build_traversability_map", kBlock);
  const std::vector<mp2p_icp_hip::PosedFrame> posed = session_map_frames(set, map_index);
  TraversabilityMap m;
  m.resolution = opt.resolution;
  m.z_quantum = opt.z_quantum;
  m.clearance_q = opt.clearanceQ();
  m.step_q = opt.stepQ();
  m.rise_q = opt.riseQ();
  m.min_points_per_cell = opt.min_points_per_cell;
  m.min_obstacle_points = opt.min_obstacle_points;
  m.frames = posed.size();
  const std::vector<mh_map_frame> frames = mp2p_icp_hip::to_map_frames(posed);
  for (const auto& f : posed) m.points += f.n;
  if (!m.points)
    throw std::runtime_error("build_traversability_map: the key-frames hold no points for target map '" + set.maps[map_index].name + "'");
  if (!ctx) ctx = DeviceContext::Default();
  using clock = std::chrono::steady_clock;
  auto since = [](clock::time_point t0) { return std::chrono::duration<double>(clock::now() - t0).count(); };
  int32_t lo[2] = {0, 0}, hi[2] = {0, 0};
  uint64_t n_in = 0;
  auto t0 = clock::now();
  check(mh_elev_bounds_frames(ctx->get(), frames.data(), frames.size(), MH_MEM_HOST, (float)opt.resolution, (float)opt.max_range,
                              max_points_per_pass, lo, hi, &n_in), "mh_elev_bounds_frames");
  m.seconds_bounds = since(t0);
  if (!n_in)
    throw std::runtime_error("build_traversability_map: no point of the key-frames is finite and inside max_range and the index range: the map is empty");
  const int64_t mg = opt.margin_cells;
  const int64_t nx = (int64_t)hi[0] - lo[0] + 1 + 2 * mg, ny = (int64_t)hi[1] - lo[1] + 1 + 2 * mg;
  if (nx * ny > (int64_t)1 << 26) throw std::runtime_error("build_traversability_map: the map would exceed 2^26 cells: raise traversability: resolution");
  m.x0 = (int32_t)(lo[0] - mg);
  m.y0 = (int32_t)(lo[1] - mg);
  m.nx = (uint32_t)nx;
  m.ny = (uint32_t)ny;
  mh_elev_params p{};
  p.resolution = (float)opt.resolution;
  p.z_quantum = (float)opt.z_quantum;
  p.max_range = (float)opt.max_range;
  p.x0 = m.x0; p.y0 = m.y0; p.nx = m.nx; p.ny = m.ny;
  p.clearance_q = m.clearance_q;
  p.step_q = m.step_q;
  mh_elev* raw = nullptr;
  check(mh_elev_create(ctx->get(), &p, &raw), "mh_elev_create");
  std::unique_ptr<mh_elev, mh_status (*)(mh_elev*)> elev(raw, &mh_elev_destroy);
  t0 = clock::now();
  check(mh_elev_add_frames(elev.get(), frames.data(), frames.size(), MH_MEM_HOST, max_points_per_pass), "mh_elev_add_frames");
  m.seconds_add = since(t0);
  t0 = clock::now();
  check(mh_elev_mark_frames(elev.get(), frames.data(), frames.size(), MH_MEM_HOST, max_points_per_pass), "mh_elev_mark_frames");
  m.seconds_mark = since(t0);
  const size_t n = (size_t)m.nx * m.ny;
  m.ground.resize(n); m.top.resize(n); m.count.resize(n); m.obstacle_count.resize(n); m.relief1.resize(n); m.reliefR.resize(n);
  t0 = clock::now();
  check(mh_elev_relief(elev.get(), 1, opt.min_points_per_cell, m.relief1.data()), "mh_elev_relief");
  check(mh_elev_relief(elev.get(), opt.slope_radius_cells, opt.min_points_per_cell, m.reliefR.data()), "mh_elev_relief");
  m.seconds_relief = since(t0);
  check(mh_elev_download(elev.get(), m.ground.data(), m.count.data(), m.obstacle_count.data(), m.top.data()), "mh_elev_download");
  mh_elev_info info;
  check(mh_elev_get_info(elev.get(), &info), "mh_elev_get_info");
  m.points_counted = info.n_counted;
  m.points_left_out = info.n_left_out;
  m.points_outside_window = info.n_outside_window;
  traversability_classify(m);
  return m;
}

}  // namespace mola_hip
