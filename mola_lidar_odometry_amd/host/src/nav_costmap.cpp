// nav_costmap.cpp -- see mola_lidar_odometry_hip/NavCostmap.h.  Host logic only: the device is reached through
// include/molahip_nav.h.
#include "mola_lidar_odometry_hip/NavCostmap.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "config_block.h"
#include "map_files.h"

namespace mola_hip {

namespace {

const char* const kBlock = "costmap";

[[noreturn]] void bad(const std::string& key, const std::string& what) { bad_option(kBlock, key, what); }

uint8_t reach_byte(uint8_t reached) { return reached ? 255 : 0; }

// a plane of the costmap at `prefix` from its image
std::vector<uint8_t> window_plane(const std::string& path, uint32_t nx, uint32_t ny, const std::string& prefix) {
  std::vector<uint8_t> v;
  if (!pgm_plane(slurp("read_costmap", path), nx, ny, nx, ny, v))
    throw std::runtime_error("read_costmap: '" + path + "' is not an image of the window of '" + prefix + ".pgm'");
  return v;
}

// rule 3 for one axis; false when the translation has no cell
bool cell_index(double t, double resolution, int64_t& out) {
  const float s = (float)t * (1.0f / (float)resolution);
  if (!std::isfinite(s) || !(std::fabs(s) < 1.0e6f)) return false;
  out = (int64_t)std::floor(s);
  return true;
}

// the cell of a pose relative to the window, or (-1, -1)
void cell_of(const CostmapBase& b, const Pose12& T, int32_t& col, int32_t& row) {
  int64_t ix = 0, iy = 0;
  col = row = -1;
  if (!cell_index(T[3], b.resolution, ix) || !cell_index(T[7], b.resolution, iy)) return;
  const int64_t cx = ix - b.x0, cy = iy - b.y0;
  if (cx < 0 || cy < 0 || cx >= (int64_t)b.nx || cy >= (int64_t)b.ny) return;
  col = (int32_t)cx;
  row = (int32_t)cy;
}

void check_base(const CostmapBase& b, const char* who) {
  if (b.nx == 0 || b.ny == 0 || b.bytes.size() != (size_t)b.nx * b.ny) throw std::runtime_error(std::string(who) + ": the base plane needs ny * nx bytes");
  if (!(b.resolution > 0.0) || !std::isfinite(b.resolution)) throw std::runtime_error(std::string(who) + ": the base plane's resolution must be finite and > 0");
}

}  // namespace

// ================================================================== options
NavCostmapOptions NavCostmapOptions::FromConfig(const Config& cfg) {
  NavCostmapOptions o;
  if (cfg.has(kBlock) && !cfg[kBlock].isNull()) {
    const ConfigBlock c(cfg[kBlock], kBlock);
    c.knownKeys({"source", "inscribed_radius", "inflation_radius", "cost_scaling", "unknown_is_obstacle", "reach_from"});
    c.text("source", o.source);
    c.number("inscribed_radius", o.inscribed_radius);
    c.number("inflation_radius", o.inflation_radius);
    c.number("cost_scaling", o.cost_scaling);
    c.boolean("unknown_is_obstacle", o.unknown_is_obstacle);
    c.text("reach_from", o.reach_from);
  }
  o.validate();
  return o;
}

void NavCostmapOptions::validate() const {
  if (source != "traversability" && source != "occupancy_grid") bad("source", "must be traversability or occupancy_grid");
  if (!(inscribed_radius >= 0.0) || !std::isfinite(inscribed_radius)) bad("inscribed_radius", "must be finite and >= 0");
  if (!(inflation_radius >= inscribed_radius) || !std::isfinite(inflation_radius)) bad("inflation_radius", "must be finite and >= inscribed_radius");
  if (!(cost_scaling > 0.0) || !std::isfinite(cost_scaling)) bad("cost_scaling", "must be finite and > 0");
  if (reach_from != "keyframes" && reach_from != "first" && reach_from != "none") bad("reach_from", "must be keyframes, first or none");
}

uint32_t NavCostmapOptions::maxCells(double resolution) const {
  validate();
  if (!(resolution > 0.0) || !std::isfinite(resolution)) throw std::runtime_error("costmap: the source map's resolution must be finite and > 0");
  const double r = std::ceil(inflation_radius / resolution);
  if (!(r <= (double)MH_NAV_MAX_CELLS)) bad("inflation_radius", "spans more than 255 cells of the source map (" + g9(inflation_radius) + " m at " + g9(resolution) + " m per cell)");
  return (uint32_t)r;
}

// ================================================================== host rules
CostmapBase costmap_base(const TraversabilityMap& m) {
  CostmapBase b;
  b.x0 = m.x0; b.y0 = m.y0; b.nx = m.nx; b.ny = m.ny;
  b.resolution = m.resolution;
  b.bytes = m.cost;
  check_base(b, "costmap_base");
  return b;
}

CostmapBase costmap_base(const OccupancyGrid& g) {
  CostmapBase b;
  b.x0 = g.x0; b.y0 = g.y0; b.nx = g.nx; b.ny = g.ny;
  b.resolution = g.resolution;
  b.bytes.resize(g.cells.size());
  for (size_t i = 0; i < g.cells.size(); i++) {
    const int8_t c = g.cells[i];
    if (c != kGridOccupied && c != kGridFree && c != kGridUnknown) throw std::runtime_error("costmap_base: a grid cell is neither occupied, free nor unknown");
    b.bytes[i] = c == kGridOccupied ? (uint8_t)MH_NAV_LETHAL : c == kGridUnknown ? (uint8_t)MH_NAV_UNKNOWN : (uint8_t)0;
  }
  check_base(b, "costmap_base");
  return b;
}

std::vector<uint8_t> inflation_table(const NavCostmapOptions& opt, double resolution) {
  const uint32_t R = opt.maxCells(resolution);
  std::vector<uint8_t> t((size_t)R * R + 1, 0);
  for (uint32_t d2 = 1; d2 <= R * R; d2++) {
    const double d = std::sqrt((double)d2) * resolution;
    if (d <= opt.inscribed_radius) t[d2] = 253;
    else if (d <= opt.inflation_radius) t[d2] = (uint8_t)std::floor(252.0 * std::exp(-opt.cost_scaling * (d - opt.inscribed_radius)));
  }
  return t;
}

std::vector<int32_t> costmap_seeds(const CostmapBase& base, const std::vector<Pose12>& poses, const std::string& reach_from) {
  if (reach_from != "keyframes" && reach_from != "first" && reach_from != "none") bad("reach_from", "must be keyframes, first or none");
  const size_t n = reach_from == "none" ? 0 : reach_from == "first" ? std::min<size_t>(poses.size(), 1) : poses.size();
  std::vector<int32_t> seeds(2 * n);
  for (size_t k = 0; k < n; k++) cell_of(base, poses[k], seeds[2 * k], seeds[2 * k + 1]);
  return seeds;
}

void costmap_summarise(NavCostmap& c, const std::vector<Pose12>& poses) {
  const size_t n = (size_t)c.nx * c.ny;
  if (n == 0 || c.cost.size() != n || c.reach.size() != n || (!c.d2.empty() && c.d2.size() != n))
    throw std::runtime_error("costmap_summarise: cost and reach need ny * nx entries each, d2 as many or none");
  c.cells_lethal = c.cells_inscribed = c.cells_inflated = c.cells_free = c.cells_unknown = c.cells_reached = c.cells_unreachable_free = 0;
  for (size_t i = 0; i < n; i++) {
    const uint8_t v = c.cost[i];
    if (v == MH_NAV_UNKNOWN) c.cells_unknown++;
    else if (v == MH_NAV_LETHAL) c.cells_lethal++;
    else if (v == 253) c.cells_inscribed++;
    else {
      if (!c.d2.empty()) (c.d2[i] != MH_NAV_FAR ? c.cells_inflated : c.cells_free)++;
      if (!c.reach[i]) c.cells_unreachable_free++;
    }
    if (c.reach[i]) c.cells_reached++;
  }
  CostmapBase w;
  w.x0 = c.x0; w.y0 = c.y0; w.nx = c.nx; w.ny = c.ny;
  w.resolution = c.resolution;
  c.keyframe_d2.assign(poses.size(), (uint16_t)MH_NAV_FAR);
  c.keyframe_cost.assign(poses.size(), (uint8_t)MH_NAV_UNKNOWN);
  c.keyframe_reached.assign(poses.size(), 0);
  c.keyframes_blocked = 0;
  c.trajectory_min_clearance_m = -1.0;
  uint32_t best = MH_NAV_FAR;
  for (size_t k = 0; k < poses.size(); k++) {
    int32_t col, row;
    cell_of(w, poses[k], col, row);
    if (col >= 0) {
      const size_t i = (size_t)row * c.nx + (size_t)col;
      if (!c.d2.empty()) c.keyframe_d2[k] = c.d2[i];
      c.keyframe_cost[k] = c.cost[i];
      c.keyframe_reached[k] = c.reach[i] ? 1 : 0;
    }
    if (c.keyframe_cost[k] >= 253) c.keyframes_blocked++;
    best = std::min<uint32_t>(best, c.keyframe_d2[k]);
  }
  if (best != MH_NAV_FAR) c.trajectory_min_clearance_m = std::sqrt((double)best) * c.resolution;
}

void write_costmap(const NavCostmap& c, const std::string& prefix) {
  const size_t n = (size_t)c.nx * c.ny;
  if (n == 0 || c.cost.size() != n || c.reach.size() != n) throw std::runtime_error("write_costmap: the costmap holds no cells");
  OccupancyGrid g;  // the trinary pair is OccupancyGrid.h's, written by its writer
  g.x0 = c.x0; g.y0 = c.y0; g.nx = c.nx; g.ny = c.ny;
  g.resolution = c.resolution;
  g.cells.resize(n);
  for (size_t i = 0; i < n; i++) g.cells[i] = c.cost[i] == MH_NAV_UNKNOWN ? kGridUnknown : c.cost[i] >= 253 ? kGridOccupied : kGridFree;
  write_occupancy_grid(g, prefix);
  const char* const who = "write_costmap";
  const std::string name = base_name(prefix);
  write_file(who, prefix + ".yaml", "cost_image: " + name + "_cost.pgm\nreach_image: " + name + "_reach.pgm\ninscribed_radius: " + g9(c.inscribed_radius) +
                                        "\ninflation_radius: " + g9(c.inflation_radius) + "\n", std::ios::app);
  write_file(who, prefix + "_cost.pgm", pgm_bytes(c.cost.data(), c.nx, c.ny), std::ios::trunc);
  write_file(who, prefix + "_reach.pgm", pgm_bytes(c.reach.data(), c.nx, c.ny, reach_byte), std::ios::trunc);
}

NavCostmap read_costmap(const std::string& prefix) {
  const OccupancyGrid g = read_occupancy_grid(prefix);  // the window, the resolution, the trinary cells
  NavCostmap c;
  c.x0 = g.x0; c.y0 = g.y0; c.nx = g.nx; c.ny = g.ny;
  c.resolution = g.resolution;
  const std::string yaml = slurp("read_costmap", prefix + ".yaml"), dir = dir_of(prefix);
  std::string cost_name, reach_name, inscribed, inflation;
  yaml_line(yaml, "cost_image: ", cost_name);
  yaml_line(yaml, "reach_image: ", reach_name);
  if (cost_name.empty() || reach_name.empty() || !yaml_line(yaml, "inscribed_radius:", inscribed) || !yaml_line(yaml, "inflation_radius:", inflation))
    throw std::runtime_error("read_costmap: '" + prefix + ".yaml' lacks cost_image, reach_image, inscribed_radius or inflation_radius");
  c.inscribed_radius = strtod(inscribed.c_str(), nullptr);
  c.inflation_radius = strtod(inflation.c_str(), nullptr);
  c.cost = window_plane(dir + cost_name, c.nx, c.ny, prefix);
  c.reach = window_plane(dir + reach_name, c.nx, c.ny, prefix);
  for (size_t i = 0; i < c.cost.size(); i++) {
    const int8_t want = c.cost[i] == MH_NAV_UNKNOWN ? kGridUnknown : c.cost[i] >= 253 ? kGridOccupied : kGridFree;
    if (g.cells[i] != want) throw std::runtime_error("read_costmap: '" + dir + cost_name + "' disagrees with the trinary image '" + prefix + ".pgm'");
    if (c.reach[i] != 0 && c.reach[i] != 255) throw std::runtime_error("read_costmap: '" + dir + reach_name + "' holds a byte that is neither 0 nor 255");
    c.reach[i] = c.reach[i] ? 1 : 0;
  }
  costmap_summarise(c, {});
  return c;
}

// ================================================================== the whole thing
NavCostmap build_costmap(const CostmapBase& base, const std::vector<Pose12>& poses, const NavCostmapOptions& opt, std::shared_ptr<DeviceContext> ctx) {
  using mp2p_icp_hip::check;
  opt.validate();
  check_base(base, "build_costmap");
  if ((uint64_t)base.nx * base.ny > (1ull << 26)) throw std::runtime_error("build_costmap: the source map exceeds 2^26 cells");
  const std::vector<uint8_t> table = inflation_table(opt, base.resolution);
  const std::vector<int32_t> seeds = costmap_seeds(base, poses, opt.reach_from);
  NavCostmap c;
  c.x0 = base.x0; c.y0 = base.y0; c.nx = base.nx; c.ny = base.ny;
  c.resolution = base.resolution;
  c.inscribed_radius = opt.inscribed_radius;
  c.inflation_radius = opt.inflation_radius;
  c.max_cells = opt.maxCells(base.resolution);
  c.unknown_is_obstacle = opt.unknown_is_obstacle;
  if (!ctx) ctx = DeviceContext::Default();
  using clock = std::chrono::steady_clock;
  auto since = [](clock::time_point t0) { return std::chrono::duration<double>(clock::now() - t0).count(); };
  mh_nav* raw = nullptr;
  check(mh_nav_create(ctx->get(), c.nx, c.ny, &raw), "mh_nav_create");
  std::unique_ptr<mh_nav, mh_status (*)(mh_nav*)> nav(raw, &mh_nav_destroy);
  auto t0 = clock::now();
  check(mh_nav_set_base(nav.get(), base.bytes.data(), MH_MEM_HOST), "mh_nav_set_base");
  check(mh_nav_inflate(nav.get(), c.max_cells, opt.unknown_is_obstacle ? 1 : 0, table.data(), table.size()), "mh_nav_inflate");
  c.seconds_inflate = since(t0);
  t0 = clock::now();
  check(mh_nav_reach(nav.get(), seeds.empty() ? nullptr : seeds.data(), seeds.size() / 2, kCostmapPassableBelow), "mh_nav_reach");
  c.seconds_reach = since(t0);
  const size_t n = (size_t)c.nx * c.ny;
  c.d2.resize(n); c.cost.resize(n); c.reach.resize(n);
  check(mh_nav_download(nav.get(), c.d2.data(), c.cost.data(), c.reach.data()), "mh_nav_download");
  mh_nav_info info;
  check(mh_nav_get_info(nav.get(), &info), "mh_nav_get_info");
  c.seeds = seeds.size() / 2;
  c.seeds_blocked = info.n_seeds_blocked;
  c.seeds_outside = info.n_seeds_outside;
  c.sweeps = info.n_sweeps;
  costmap_summarise(c, poses);
  if (c.cells_reached != info.n_reached) throw std::runtime_error("build_costmap: the reach plane and mh_nav_info::n_reached disagree");
  return c;
}

NavCostmap build_costmap_from_keyframes(const molahip_host::KeyFrameSet& set, const Config& pipeline, std::shared_ptr<DeviceContext> ctx) {
  const NavCostmapOptions opt = NavCostmapOptions::FromConfig(pipeline);
  std::vector<Pose12> poses(set.frames.size());
  for (size_t k = 0; k < set.frames.size(); k++) std::copy(set.frames[k].pose, set.frames[k].pose + 12, poses[k].begin());
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  CostmapBase base;
  if (opt.source == "traversability") {
    const TraversabilityOptions topt = TraversabilityOptions::FromConfig(pipeline);
    opt.maxCells(topt.resolution);  // (refused before a device is asked for and the source map is built)
    if (!ctx) ctx = DeviceContext::Default();
    base = costmap_base(build_traversability_map(set, topt, ctx));
  } else {
    const OccupancyGridOptions gopt = OccupancyGridOptions::FromConfig(pipeline);
    opt.maxCells(gopt.resolution);
    if (!ctx) ctx = DeviceContext::Default();
    base = costmap_base(build_occupancy_grid(set, gopt, ctx));
  }
  const double seconds_source = std::chrono::duration<double>(clock::now() - t0).count();
  NavCostmap c = build_costmap(base, poses, opt, ctx);
  c.seconds_source = seconds_source;
  return c;
}

}  // namespace mola_hip
