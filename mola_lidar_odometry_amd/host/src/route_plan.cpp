// route_plan.cpp -- see mola_lidar_odometry_hip/RoutePlan.h.  Host logic only: the device is reached through
// include/molahip_plan.h.
#include "mola_lidar_odometry_hip/RoutePlan.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <stdexcept>

#include "config_block.h"
#include "map_files.h"

namespace mola_hip {

namespace {

const char* const kBlock = "route";

[[noreturn]] void bad(const std::string& key, const std::string& what) { bad_option(kBlock, key, what); }

void check_costmap(const NavCostmap& c, const char* who) {
  const size_t n = (size_t)c.nx * c.ny;
  if (n == 0 || c.cost.size() != n || (!c.d2.empty() && c.d2.size() != n))
    throw std::runtime_error(std::string(who) + ": the costmap needs ny * nx cost bytes, and as many d2 or none");
  if (!(c.resolution > 0.0) || !std::isfinite(c.resolution)) throw std::runtime_error(std::string(who) + ": the costmap's resolution must be finite and > 0");
}

void integer_key(const ConfigBlock& c, const char* k, int64_t& v) {
  double d = (double)v;
  c.number(k, d);
  if (!(d >= -1.0) || !(d <= 4294967295.0) || d != std::floor(d)) c.bad(k, "must be an integer >= -1");
  v = (int64_t)d;
}

}  // namespace

// ================================================================== options
RouteOptions RouteOptions::FromConfig(const Config& cfg) {
  RouteOptions o;
  if (cfg.has(kBlock) && !cfg[kBlock].isNull()) {
    const ConfigBlock c(cfg[kBlock], kBlock);
    c.knownKeys({"start_x", "start_y", "goal_x", "goal_y", "start_keyframe", "goal_keyframe", "neutral_price", "cost_factor", "max_route_cells"});
    for (const auto& kv : {std::make_pair("start_x", &o.start_x), std::make_pair("start_y", &o.start_y), std::make_pair("goal_x", &o.goal_x),
                           std::make_pair("goal_y", &o.goal_y)}) {
      c.number(kv.first, *kv.second);
      if (c.value(kv.first) && !std::isfinite(*kv.second)) c.bad(kv.first, "must be finite");
    }
    integer_key(c, "start_keyframe", o.start_keyframe);
    integer_key(c, "goal_keyframe", o.goal_keyframe);
    c.count("neutral_price", o.neutral_price);
    c.number("cost_factor", o.cost_factor);
    c.count("max_route_cells", o.max_route_cells);
  }
  o.validate();
  return o;
}

void RouteOptions::validate() const {
  const bool sx = start_x == start_x, sy = start_y == start_y, gx = goal_x == goal_x, gy = goal_y == goal_y;
  if (sx != sy) bad(sx ? "start_y" : "start_x", "must be given when the other coordinate of the start is");
  if (gx != gy) bad(gx ? "goal_y" : "goal_x", "must be given when the other coordinate of the goal is");
  if ((sx && !std::isfinite(start_x)) || (sy && !std::isfinite(start_y))) bad(std::isfinite(start_x) ? "start_y" : "start_x", "must be finite");
  if ((gx && !std::isfinite(goal_x)) || (gy && !std::isfinite(goal_y))) bad(std::isfinite(goal_x) ? "goal_y" : "goal_x", "must be finite");
  if (start_keyframe < -1) bad("start_keyframe", "must be an integer >= -1");
  if (goal_keyframe < -1) bad("goal_keyframe", "must be an integer >= -1");
  if (neutral_price < 1) bad("neutral_price", "must be an integer >= 1");
  if (!(cost_factor >= 0.0) || !std::isfinite(cost_factor)) bad("cost_factor", "must be finite and >= 0");
  if (max_route_cells < 1) bad("max_route_cells", "must be an integer >= 1");
}

// ================================================================== host rules
std::vector<uint16_t> route_price_table(const RouteOptions& opt) {
  opt.validate();
  std::vector<uint16_t> t(kCostmapPassableBelow);
  for (uint32_t c = 0; c < kCostmapPassableBelow; c++) {
    const double p = (double)opt.neutral_price + std::floor(opt.cost_factor * (double)c);
    if (!(p <= 65535.0)) bad(opt.neutral_price > 65535u ? "neutral_price" : "cost_factor", "gives cost " + std::to_string(c) + " a price above 65535");
    t[c] = (uint16_t)p;
  }
  return t;
}

void route_check_window(const std::vector<uint16_t>& price, uint64_t n_cells) {
  uint64_t top = 0;
  for (uint16_t p : price) top = std::max<uint64_t>(top, p);
  if (top == 0 || n_cells == 0) throw std::runtime_error("route: a price table of entries >= 1 and a window of at least one cell are needed");
  if ((n_cells - 1) * 14ull * top < 0xFFFFFFFFull) return;
  const uint64_t admit = 0xFFFFFFFEull / (14ull * top) + 1ull;
  throw std::runtime_error("route: neutral_price and cost_factor give prices up to " + std::to_string(top) + ", which admit a window of at most " +
                           std::to_string(admit) + " cells; this one has " + std::to_string(n_cells) + " (the field is 32 bits wide)");
}

bool route_cell(const NavCostmap& c, double x, double y, int32_t& col, int32_t& row) {
  CostmapBase w;  // (costmap_seeds reads the window and the resolution only)
  w.x0 = c.x0; w.y0 = c.y0; w.nx = c.nx; w.ny = c.ny;
  w.resolution = c.resolution;
  const std::vector<int32_t> s = costmap_seeds(w, {Pose12{1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, 0}}, "keyframes");
  col = s[0];
  row = s[1];
  return col >= 0;
}

void route_summarise(RoutePlan& r, const NavCostmap& c) {
  check_costmap(c, "route_summarise");
  if (r.cells.size() % 2) throw std::runtime_error("route_summarise: the route's cells are (column, row) pairs");
  const size_t n = r.cells.size() / 2;
  r.xy.resize(2 * n);
  r.length_m = 0;
  r.max_cost = 0;
  r.min_clearance_m = -1.0;
  uint32_t best = MH_NAV_FAR;
  for (size_t k = 0; k < n; k++) {
    const int32_t col = r.cells[2 * k], row = r.cells[2 * k + 1];
    if (col < 0 || row < 0 || (uint32_t)col >= c.nx || (uint32_t)row >= c.ny) throw std::runtime_error("route_summarise: a route cell lies outside the window");
    r.xy[2 * k] = ((double)c.x0 + (double)col + 0.5) * c.resolution;
    r.xy[2 * k + 1] = ((double)c.y0 + (double)row + 0.5) * c.resolution;
    const size_t i = (size_t)row * c.nx + (size_t)col;
    r.max_cost = std::max<uint32_t>(r.max_cost, c.cost[i]);
    if (!c.d2.empty()) best = std::min<uint32_t>(best, c.d2[i]);
    if (k > 0) {
      const int32_t dx = col - r.cells[2 * k - 2], dy = row - r.cells[2 * k - 1];
      if (dx < -1 || dx > 1 || dy < -1 || dy > 1 || (dx == 0 && dy == 0)) throw std::runtime_error("route_summarise: two route cells in a row are no neighbours");
      r.length_m += (dx != 0 && dy != 0) ? c.resolution * std::sqrt(2.0) : c.resolution;
    }
  }
  if (best != MH_NAV_FAR) r.min_clearance_m = std::sqrt((double)best) * c.resolution;
}

void write_route(const RoutePlan& r, const NavCostmap& c, const std::string& prefix, const std::string& stem) {
  check_costmap(c, "write_route");
  if (r.xy.size() != r.cells.size()) throw std::runtime_error("write_route: the route's cells and its points differ in number");
  const char* const who = "write_route";
  std::string text;
  char line[64];
  for (size_t k = 0; k + 1 < r.xy.size(); k += 2) {
    snprintf(line, sizeof line, "%.9g %.9g\n", r.xy[k], r.xy[k + 1]);
    text += line;
  }
  std::vector<uint8_t> px(c.cost.size());
  for (size_t i = 0; i < px.size(); i++) px[i] = c.cost[i] == MH_NAV_UNKNOWN ? 205 : c.cost[i] >= 253 ? 0 : 254;  // (the trinary image's bytes)
  for (size_t k = 0; k + 1 < r.cells.size(); k += 2) {
    const int32_t col = r.cells[k], row = r.cells[k + 1];
    if (col < 0 || row < 0 || (uint32_t)col >= c.nx || (uint32_t)row >= c.ny) throw std::runtime_error("write_route: a route cell lies outside the window");
    px[(size_t)row * c.nx + (size_t)col] = 100;
  }
  write_file(who, prefix + stem + ".txt", text, std::ios::trunc);
  write_file(who, prefix + stem + ".pgm", pgm_bytes(px.data(), c.nx, c.ny), std::ios::trunc);
}

// ================================================================== the whole thing
RoutePlan plan_route(const NavCostmap& c, const RouteOptions& opt, std::shared_ptr<DeviceContext> ctx) {
  using mp2p_icp_hip::check;
  opt.validate();
  check_costmap(c, "plan_route");
  if (!opt.hasStart()) bad("start_x", "and start_y are needed where no key-frames are at hand");
  if (!opt.hasGoal()) bad("goal_x", "and goal_y are needed where no key-frames are at hand");
  const size_t n = (size_t)c.nx * c.ny;
  if ((uint64_t)n > (1ull << 26)) throw std::runtime_error("plan_route: the costmap exceeds 2^26 cells");
  const std::vector<uint16_t> price = route_price_table(opt);
  route_check_window(price, n);
  RoutePlan r;
  const bool s_in = route_cell(c, opt.start_x, opt.start_y, r.start_col, r.start_row);
  const bool g_in = route_cell(c, opt.goal_x, opt.goal_y, r.goal_col, r.goal_row);
  if (!s_in) r.status = "start_outside";
  else if (c.cost[(size_t)r.start_row * c.nx + (size_t)r.start_col] >= kCostmapPassableBelow) r.status = "start_blocked";
  else if (!g_in) r.status = "goal_outside";
  else if (c.cost[(size_t)r.goal_row * c.nx + (size_t)r.goal_col] >= kCostmapPassableBelow) r.status = "goal_blocked";
  if (!r.status.empty()) return r;
  if (!ctx) ctx = DeviceContext::Default();
  using clock = std::chrono::steady_clock;
  auto since = [](clock::time_point t0) { return std::chrono::duration<double>(clock::now() - t0).count(); };
  mh_plan* raw = nullptr;
  check(mh_plan_create(ctx->get(), c.nx, c.ny, &raw), "mh_plan_create");
  std::unique_ptr<mh_plan, mh_status (*)(mh_plan*)> plan(raw, &mh_plan_destroy);
  check(mh_plan_set_cost(plan.get(), c.cost.data(), MH_MEM_HOST), "mh_plan_set_cost");
  auto t0 = clock::now();
  const int32_t goal[2] = {r.goal_col, r.goal_row}, start[2] = {r.start_col, r.start_row};
  check(mh_plan_field(plan.get(), goal, 1, kCostmapPassableBelow, price.data(), price.size()), "mh_plan_field");
  r.seconds_field = since(t0);
  r.field.resize(n);
  check(mh_plan_download(plan.get(), r.field.data()), "mh_plan_download");
  mh_plan_info info;
  check(mh_plan_get_info(plan.get(), &info), "mh_plan_get_info");
  r.sweeps = info.n_sweeps;
  r.tile_runs = info.n_tile_runs;
  r.cells_with_field = info.n_reached;
  r.cost_to_go = r.field[(size_t)r.start_row * c.nx + (size_t)r.start_col];
  if (r.cost_to_go == MH_PLAN_UNREACHED) {
    r.status = "unreachable";
    return r;
  }
  const uint32_t cap = (uint32_t)std::min<uint64_t>(opt.max_route_cells, n);  // (a route visits a cell at most once)
  r.cells.resize((size_t)cap * 2);
  uint32_t len = 0;
  t0 = clock::now();
  check(mh_plan_trace(plan.get(), start, 1, cap, r.cells.data(), &len), "mh_plan_trace");
  r.seconds_trace = since(t0);
  r.status = len == MH_PLAN_TRUNCATED ? "truncated" : "found";
  r.cells.resize((size_t)(len == MH_PLAN_TRUNCATED ? cap : len) * 2);
  route_summarise(r, c);
  return r;
}

RouteFromKeyframes plan_route_from_keyframes(const molahip_host::KeyFrameSet& set, const Config& pipeline, std::shared_ptr<DeviceContext> ctx) {
  RouteOptions opt = RouteOptions::FromConfig(pipeline);
  (void)route_price_table(opt);  // (a bad block is refused before the costmap is built)
  auto pick = [&](int64_t k, const char* key, double& x, double& y) {
    if (set.frames.empty()) bad(key, "names a key-frame of an empty set");
    const int64_t i = k < 0 ? (int64_t)set.frames.size() - 1 : k;
    if (i >= (int64_t)set.frames.size()) bad(key, "is " + std::to_string(k) + ", the set has " + std::to_string(set.frames.size()) + " key-frames");
    x = set.frames[(size_t)i].pose[3];
    y = set.frames[(size_t)i].pose[7];
  };
  if (!opt.hasStart()) pick(opt.start_keyframe, "start_keyframe", opt.start_x, opt.start_y);
  if (!opt.hasGoal()) pick(opt.goal_keyframe, "goal_keyframe", opt.goal_x, opt.goal_y);
  if (!ctx) ctx = DeviceContext::Default();
  RouteFromKeyframes out;
  out.costmap = build_costmap_from_keyframes(set, pipeline, ctx);
  if (!std::isfinite(opt.start_x) || !std::isfinite(opt.start_y)) opt.start_x = opt.start_y = 1.0e30;  // (a pose that is not finite has no cell)
  if (!std::isfinite(opt.goal_x) || !std::isfinite(opt.goal_y)) opt.goal_x = opt.goal_y = 1.0e30;
  out.route = plan_route(out.costmap, opt, ctx);
  return out;
}

}  // namespace mola_hip
