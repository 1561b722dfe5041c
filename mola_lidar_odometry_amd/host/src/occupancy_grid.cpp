// occupancy_grid.cpp -- see mola_lidar_odometry_hip/OccupancyGrid.h.  Host logic only: the device is reached through the three
// CVoxelMap methods over include/molahip_occgrid.h.
#include "mola_lidar_odometry_hip/OccupancyGrid.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>

#include "mola_lidar_odometry_hip/LidarOdometry.h"

namespace mola_hip {

namespace {

const char* const kBlock = "occupancy_grid";

[[noreturn]] void bad(const std::string& key, const std::string& what) { throw std::runtime_error(std::string(kBlock) + ": " + key + " " + what); }

void number(const Config& c, const char* k, double& v) {
  if (!c.has(k) || c[k].isNull()) return;
  const std::string s = c[k].asString();
  char* end = nullptr;
  v = strtod(s.c_str(), &end);
  if (end == s.c_str() || *end != '\0') bad(k, "must be a number");
}

void count(const Config& c, const char* k, uint32_t& v) {
  double d = v;
  number(c, k, d);
  if (!(d >= 0.0) || !(d <= 4294967295.0) || d != std::floor(d)) bad(k, "must be an integer >= 0");
  v = (uint32_t)d;
}

void boolean(const Config& c, const char* k, bool& v) {
  if (!c.has(k) || c[k].isNull()) return;
  const std::string s = c[k].asString();
  if (s == "true" || s == "True" || s == "1" || s == "yes") v = true;
  else if (s == "false" || s == "False" || s == "0" || s == "no") v = false;
  else bad(k, "must be true or false");
}

bool in01(double p) { return p > 0.0 && p < 1.0; }

std::string g9(double v) {
  char buf[64];
  snprintf(buf, sizeof(buf), "%.9g", v);
  return buf;
}

std::string base_name(const std::string& path) {
  const size_t s = path.find_last_of('/');
  return s == std::string::npos ? path : path.substr(s + 1);
}

}  // namespace

// ================================================================== options
OccupancyGridOptions OccupancyGridOptions::FromConfig(const Config& cfg) {
  OccupancyGridOptions o;
  if (cfg.has(kBlock) && !cfg[kBlock].isNull()) {
    const Config& c = cfg[kBlock];
    static const char* const keys[] = {"resolution", "prob_hit", "prob_miss", "clamp_min", "clamp_max", "occupied_threshold",
                                       "ray_trace_free_space", "max_range", "decimation", "update_rule", "target_map", "z_min", "z_max",
                                       "margin_cells"};
    for (const auto& kv : c.map)
      if (std::find_if(std::begin(keys), std::end(keys), [&](const char* k) { return kv.first == k; }) == std::end(keys))
        bad(kv.first, "is not a key of this block");
    number(c, "resolution", o.resolution);
    number(c, "prob_hit", o.prob_hit); number(c, "prob_miss", o.prob_miss);
    number(c, "clamp_min", o.clamp_min); number(c, "clamp_max", o.clamp_max);
    number(c, "occupied_threshold", o.occupied_threshold);
    boolean(c, "ray_trace_free_space", o.ray_trace_free_space);
    number(c, "max_range", o.max_range);
    count(c, "decimation", o.decimation);
    if (c.has("update_rule") && !c["update_rule"].isNull()) o.update_rule = c["update_rule"].asString();
    if (c.has("target_map") && !c["target_map"].isNull()) o.target_map = c["target_map"].asString();
    number(c, "z_min", o.z_min); number(c, "z_max", o.z_max);
    count(c, "margin_cells", o.margin_cells);
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
  std::string pgm = "P5\n" + std::to_string(g.nx) + " " + std::to_string(g.ny) + "\n255\n";
  const size_t head = pgm.size();
  pgm.resize(head + n);
  for (uint32_t r = 0; r < g.ny; r++) {  // row 0 of the image is the largest y
    const int8_t* src = &g.cells[(size_t)(g.ny - 1 - r) * g.nx];
    for (uint32_t c = 0; c < g.nx; c++)
      pgm[head + (size_t)r * g.nx + c] = (char)(src[c] == kGridOccupied ? 0 : src[c] == kGridFree ? 254 : 205);
  }
  const std::string yaml = "image: " + base_name(prefix) + ".pgm\nresolution: " + g9(g.resolution) + "\norigin: [" +
                           g9((double)g.x0 * g.resolution) + ", " + g9((double)g.y0 * g.resolution) +
                           ", 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n";
  const std::pair<std::string, const std::string*> files[] = {{prefix + ".pgm", &pgm}, {prefix + ".yaml", &yaml}};
  for (const auto& f : files) {
    std::ofstream out(f.first, std::ios::binary | std::ios::trunc);
    out.write(f.second->data(), (std::streamsize)f.second->size());
    out.close();
    if (!out) throw std::runtime_error("write_occupancy_grid: cannot write '" + f.first + "'");
  }
}

OccupancyGrid read_occupancy_grid(const std::string& prefix) {
  OccupancyGrid g;
  {
    const std::string path = prefix + ".yaml";
    std::ifstream in(path);
    if (!in) throw std::runtime_error("read_occupancy_grid: cannot open '" + path + "'");
    std::string line;
    double ox = 0, oy = 0;
    bool have_res = false, have_origin = false;
    while (std::getline(in, line)) {
      if (line.rfind("resolution:", 0) == 0) {
        g.resolution = strtod(line.c_str() + 11, nullptr);
        have_res = true;
      } else if (line.rfind("origin:", 0) == 0) {
        have_origin = sscanf(line.c_str() + 7, " [%lf , %lf", &ox, &oy) == 2;
      }
    }
    if (!have_res || !have_origin || !(g.resolution > 0.0)) throw std::runtime_error("read_occupancy_grid: '" + path + "' lacks resolution or origin");
    g.x0 = (int32_t)std::llround(ox / g.resolution);
    g.y0 = (int32_t)std::llround(oy / g.resolution);
  }
  const std::string path = prefix + ".pgm";
  std::ifstream in(path, std::ios::binary);
  if (!in) throw std::runtime_error("read_occupancy_grid: cannot open '" + path + "'");
  std::stringstream ss;
  ss << in.rdbuf();
  const std::string s = ss.str();
  unsigned nx = 0, ny = 0, maxv = 0;
  int used = 0;
  if (sscanf(s.c_str(), "P5\n%u %u\n%u\n%n", &nx, &ny, &maxv, &used) != 3 || maxv != 255 || used <= 0 || nx == 0 || ny == 0 ||
      s.size() != (size_t)used + (size_t)nx * ny)
    throw std::runtime_error("read_occupancy_grid: '" + path + "' is not a binary PGM written by write_occupancy_grid");
  g.nx = nx;
  g.ny = ny;
  g.cells.resize((size_t)nx * ny);
  for (uint32_t r = 0; r < ny; r++)
    for (uint32_t c = 0; c < nx; c++) {
      const unsigned char v = (unsigned char)s[(size_t)used + (size_t)r * nx + c];
      int8_t& out = g.cells[(size_t)(ny - 1 - r) * nx + c];
      if (v == 0) { out = kGridOccupied; g.cells_occupied++; }
      else if (v == 254) { out = kGridFree; g.cells_free++; }
      else if (v == 205) { out = kGridUnknown; g.cells_unknown++; }
      else throw std::runtime_error("read_occupancy_grid: '" + path + "' holds a byte that is neither 0, 254 nor 205");
    }
  return g;
}

// ================================================================== the whole thing
OccupancyGrid build_occupancy_grid(const molahip_host::KeyFrameSet& set, const OccupancyGridOptions& opt, std::shared_ptr<DeviceContext> ctx,
                                   uint64_t max_points_per_pass) {
  opt.validate();
  if (set.maps.empty()) throw std::runtime_error("build_occupancy_grid: the key-frame set names no target map");
  size_t map_index = 0;
  if (!opt.target_map.empty()) {
    while (map_index < set.maps.size() && set.maps[map_index].name != opt.target_map) map_index++;
    if (map_index == set.maps.size())
      throw std::runtime_error("build_occupancy_grid: occupancy_grid: target_map '" + opt.target_map + "' is not a target map of the key-frame set");
  }
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
