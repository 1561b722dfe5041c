// route_replan.cpp -- see mola_lidar_odometry_hip/Replan.h.  Host logic only: the device is reached through include/molahip_nav.h,
// include/molahip_plan.h and include/molahip_replan.h.
#include "mola_lidar_odometry_hip/Replan.h"

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

using clock_type = std::chrono::steady_clock;
double since(clock_type::time_point t0) { return std::chrono::duration<double>(clock_type::now() - t0).count(); }

[[noreturn]] void bad_line(uint32_t line, const std::string& what) {
  throw std::runtime_error("events: line " + std::to_string(line) + ": " + what);
}

// NavCostmap.h rule 3 for one axis; false when the value has no cell index
bool cell_index(double t, double resolution, int64_t& out) {
  const float s = (float)t * (1.0f / (float)resolution);
  if (!std::isfinite(s) || !(std::fabs(s) < 1.0e6f)) return false;
  out = (int64_t)std::floor(s);
  return true;
}

// rule 8's number: decimal, read whole by strtod, finite
bool number(const std::string& word, double& v) {
  if (word.empty() || word.find_first_of("xX_") != std::string::npos) return false;
  char* end = nullptr;
  v = std::strtod(word.c_str(), &end);
  return end == word.c_str() + word.size() && std::isfinite(v);
}

}  // namespace

// ================================================================== host rules
std::vector<ReplanEvent> parse_replan_events(const std::string& text) {
  std::vector<ReplanEvent> out;
  uint32_t line_no = 0;
  for (size_t at = 0; at <= text.size();) {
    size_t end = text.find('\n', at);
    if (end == std::string::npos) end = text.size();
    std::string line = text.substr(at, end - at);
    at = end + 1;
    line_no++;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    std::vector<std::string> words;
    for (size_t i = 0; i < line.size();) {
      while (i < line.size() && std::isspace((unsigned char)line[i])) i++;
      size_t j = i;
      while (j < line.size() && !std::isspace((unsigned char)line[j])) j++;
      if (j > i) words.push_back(line.substr(i, j - i));
      i = j;
    }
    if (words.empty()) continue;
    ReplanEvent e;
    e.line = line_no;
    size_t want = 4;
    if (words[0] == "block") e.verb = ReplanEvent::kBlock;
    else if (words[0] == "clear") e.verb = ReplanEvent::kClear;
    else if (words[0] == "at") { e.verb = ReplanEvent::kAt; want = 2; }
    else bad_line(line_no, "unknown verb '" + words[0] + "' (block, clear or at)");
    if (words.size() != 1 + want) bad_line(line_no, words[0] + " takes " + std::to_string(want) + " numbers");
    for (size_t k = 0; k < want; k++)
      if (!number(words[1 + k], e.v[k])) bad_line(line_no, "'" + words[1 + k] + "' is not a finite decimal number");
    out.push_back(e);
  }
  return out;
}

std::vector<ReplanEvent> read_replan_events(const std::string& path) { return parse_replan_events(slurp("read_replan_events", path)); }

CellRect replan_metre_rect(const NavCostmap& c, double xa, double ya, double xb, double yb) {
  if (c.nx == 0 || c.ny == 0 || !(c.resolution > 0.0) || !std::isfinite(c.resolution))
    throw std::runtime_error("replan_metre_rect: a window of at least one cell and a finite resolution > 0 are needed");
  int64_t ix[2], iy[2];
  if (!cell_index(xa, c.resolution, ix[0]) || !cell_index(xb, c.resolution, ix[1]) || !cell_index(ya, c.resolution, iy[0]) ||
      !cell_index(yb, c.resolution, iy[1]))
    throw std::runtime_error("replan_metre_rect: a corner has no cell index");
  const int64_t c0 = std::max<int64_t>(std::min(ix[0], ix[1]) - c.x0, 0), c1 = std::min<int64_t>(std::max(ix[0], ix[1]) - c.x0, (int64_t)c.nx - 1);
  const int64_t r0 = std::max<int64_t>(std::min(iy[0], iy[1]) - c.y0, 0), r1 = std::min<int64_t>(std::max(iy[0], iy[1]) - c.y0, (int64_t)c.ny - 1);
  CellRect r;
  if (c0 > c1 || r0 > r1) return r;
  r.empty = false;
  r.col0 = (uint32_t)c0; r.row0 = (uint32_t)r0;
  r.w = (uint32_t)(c1 - c0 + 1); r.h = (uint32_t)(r1 - r0 + 1);
  return r;
}

CellRect replan_grown_rect(const CellRect& r, uint32_t max_cells, uint32_t nx, uint32_t ny) {
  if (r.empty || r.w == 0 || r.h == 0 || (uint64_t)r.col0 + r.w > nx || (uint64_t)r.row0 + r.h > ny)
    throw std::runtime_error("replan_grown_rect: the rectangle is empty or leaves the window");
  CellRect g;
  g.empty = false;
  g.col0 = r.col0 > max_cells ? r.col0 - max_cells : 0u;
  g.row0 = r.row0 > max_cells ? r.row0 - max_cells : 0u;
  g.w = (uint32_t)std::min<uint64_t>((uint64_t)r.col0 + r.w + max_cells, nx) - g.col0;
  g.h = (uint32_t)std::min<uint64_t>((uint64_t)r.row0 + r.h + max_cells, ny) - g.row0;
  return g;
}

// ================================================================== the planner
RoutePlanner::RoutePlanner(CostmapBase base, std::vector<Pose12> poses, const NavCostmapOptions& copt, const RouteOptions& ropt,
                           std::shared_ptr<DeviceContext> ctx)
    : base_(std::move(base)), poses_(std::move(poses)), copt_(copt), ropt_(ropt), ctx_(std::move(ctx)) {
  using mp2p_icp_hip::check;
  copt_.validate();
  ropt_.validate();
  if (base_.nx == 0 || base_.ny == 0 || base_.bytes.size() != (size_t)base_.nx * base_.ny) throw std::runtime_error("RoutePlanner: the base plane needs ny * nx bytes");
  if (!(base_.resolution > 0.0) || !std::isfinite(base_.resolution)) throw std::runtime_error("RoutePlanner: the base plane's resolution must be finite and > 0");
  const size_t n = (size_t)base_.nx * base_.ny;
  if ((uint64_t)n > (1ull << 26)) throw std::runtime_error("RoutePlanner: the window exceeds 2^26 cells");
  if (!ropt_.hasGoal()) bad_option("route", "goal_x", "and goal_y are needed by a RoutePlanner");
  table_ = inflation_table(copt_, base_.resolution);
  max_cells_ = copt_.maxCells(base_.resolution);
  price_ = route_price_table(ropt_);
  route_check_window(price_, n);
  NavCostmap window;
  window.x0 = base_.x0; window.y0 = base_.y0; window.nx = base_.nx; window.ny = base_.ny;
  window.resolution = base_.resolution;
  if (!route_cell(window, ropt_.goal_x, ropt_.goal_y, goal_col_, goal_row_)) bad_option("route", "goal_x", "and goal_y name a point outside the window");
  // the first costmap by build_costmap itself: the reach plane and the counts are its own
  if (!ctx_) ctx_ = DeviceContext::Default();
  map_ = build_costmap(base_, poses_, copt_, ctx_);
  map_current_ = true;
  try {
    check(mh_nav_create(ctx_->get(), base_.nx, base_.ny, &nav_), "mh_nav_create");
    check(mh_plan_create(ctx_->get(), base_.nx, base_.ny, &plan_), "mh_plan_create");
    inflate();
    check(mh_plan_set_cost_from_nav(plan_, nav_), "mh_plan_set_cost_from_nav");
    const int32_t goal[2] = {goal_col_, goal_row_};
    check(mh_plan_field(plan_, goal, 1, kCostmapPassableBelow, price_.data(), price_.size()), "mh_plan_field");
  } catch (...) {
    (void)mh_plan_destroy(plan_);
    (void)mh_nav_destroy(nav_);
    throw;
  }
}

RoutePlanner::~RoutePlanner() {
  (void)mh_plan_destroy(plan_);
  (void)mh_nav_destroy(nav_);
}

void RoutePlanner::inflate() {
  using mp2p_icp_hip::check;
  check(mh_nav_set_base(nav_, base_.bytes.data(), MH_MEM_HOST), "mh_nav_set_base");
  check(mh_nav_inflate(nav_, max_cells_, copt_.unknown_is_obstacle ? 1 : 0, table_.data(), table_.size()), "mh_nav_inflate");
}

ReplanUpdate RoutePlanner::update(uint32_t col0, uint32_t row0, uint32_t w, uint32_t h, const uint8_t* bytes) {
  using mp2p_icp_hip::check;
  if (!bytes) throw std::runtime_error("RoutePlanner::update: null bytes");
  ReplanUpdate u;
  u.rect.empty = false;
  u.rect.col0 = col0; u.rect.row0 = row0; u.rect.w = w; u.rect.h = h;
  u.grown = replan_grown_rect(u.rect, max_cells_, base_.nx, base_.ny);  // (refuses an empty rectangle and one that leaves the window)
  for (uint32_t r = 0; r < h; r++) std::copy(bytes + (size_t)r * w, bytes + (size_t)(r + 1) * w, base_.bytes.begin() + ((size_t)(row0 + r) * base_.nx + col0));
  map_current_ = false;
  auto t0 = clock_type::now();
  inflate();
  u.seconds_inflate = since(t0);
  t0 = clock_type::now();
  check(mh_replan_update_cost_from_nav(plan_, nav_, u.grown.col0, u.grown.row0, u.grown.w, u.grown.h), "mh_replan_update_cost_from_nav");
  u.seconds_update = since(t0);
  check(mh_replan_get_info(plan_, &u.info), "mh_replan_get_info");
  return u;
}

ReplanUpdate RoutePlanner::fill(const CellRect& r, uint8_t byte) {
  if (r.empty) throw std::runtime_error("RoutePlanner::fill: the rectangle has no cell");
  const std::vector<uint8_t> bytes((size_t)r.w * r.h, byte);
  return update(r.col0, r.row0, r.w, r.h, bytes.data());
}

const NavCostmap& RoutePlanner::costmap() {
  using mp2p_icp_hip::check;
  if (!map_current_) {
    check(mh_nav_download(nav_, map_.d2.data(), map_.cost.data(), nullptr), "mh_nav_download");
    costmap_summarise(map_, poses_);
    map_current_ = true;
  }
  return map_;
}

mh_plan_info RoutePlanner::planInfo() const {
  mh_plan_info i;
  mp2p_icp_hip::check(mh_plan_get_info(plan_, &i), "mh_plan_get_info");
  return i;
}

RoutePlan RoutePlanner::routeFrom(double x, double y) {
  using mp2p_icp_hip::check;
  const NavCostmap& c = costmap();
  RoutePlan r;
  r.goal_col = goal_col_;
  r.goal_row = goal_row_;
  const bool s_in = route_cell(c, x, y, r.start_col, r.start_row);
  if (!s_in) r.status = "start_outside";
  else if (c.cost[(size_t)r.start_row * c.nx + (size_t)r.start_col] >= kCostmapPassableBelow) r.status = "start_blocked";
  else if (c.cost[(size_t)r.goal_row * c.nx + (size_t)r.goal_col] >= kCostmapPassableBelow) r.status = "goal_blocked";
  if (!r.status.empty()) return r;
  const mh_plan_info info = planInfo();
  r.sweeps = info.n_sweeps;
  r.tile_runs = info.n_tile_runs;
  r.cells_with_field = info.n_reached;
  const size_t n = (size_t)c.nx * c.ny;
  const uint32_t cap = (uint32_t)std::min<uint64_t>(ropt_.max_route_cells, n);  // (a route visits a cell at most once)
  // the cost-to-go of the start: a trace of one cell tells whether it is joined to the goal; the value itself is the sum of the
  // step weights along the route, which the trace rule makes equal to field[start]
  r.cells.resize((size_t)cap * 2);
  uint32_t len = 0;
  const int32_t start[2] = {r.start_col, r.start_row};
  const auto t0 = clock_type::now();
  check(mh_plan_trace(plan_, start, 1, cap, r.cells.data(), &len), "mh_plan_trace");
  r.seconds_trace = since(t0);
  if (len == 0) {
    r.cells.clear();
    r.status = "unreachable";
    return r;
  }
  r.status = len == MH_PLAN_TRUNCATED ? "truncated" : "found";
  r.cells.resize((size_t)(len == MH_PLAN_TRUNCATED ? cap : len) * 2);
  route_summarise(r, c);
  if (r.status == "found") {
    uint64_t sum = 0;
    for (size_t k = 2; k < r.cells.size(); k += 2) {
      const size_t a = (size_t)r.cells[k - 1] * c.nx + (size_t)r.cells[k - 2], b = (size_t)r.cells[k + 1] * c.nx + (size_t)r.cells[k];
      const bool diagonal = r.cells[k] != r.cells[k - 2] && r.cells[k + 1] != r.cells[k - 1];
      sum += (uint64_t)(diagonal ? MH_PLAN_STEP_DIAGONAL : MH_PLAN_STEP_ORTHOGONAL) * ((uint64_t)price_[c.cost[a]] + price_[c.cost[b]]);
    }
    r.cost_to_go = (uint32_t)sum;
  } else {  // truncated: the value is read off the field itself
    std::vector<uint32_t> field(n);
    check(mh_plan_download(plan_, field.data()), "mh_plan_download");
    r.cost_to_go = field[(size_t)r.start_row * c.nx + (size_t)r.start_col];
  }
  return r;
}

// ================================================================== the whole thing
ReplanRun replan_route_from_keyframes(const molahip_host::KeyFrameSet& set, const Config& pipeline, const std::vector<ReplanEvent>& events,
                                      std::shared_ptr<DeviceContext> ctx) {
  RouteOptions ropt = RouteOptions::FromConfig(pipeline);
  (void)route_price_table(ropt);  // (a bad block is refused before the source map is built)
  const NavCostmapOptions copt = NavCostmapOptions::FromConfig(pipeline);
  if (!ropt.hasGoal()) {
    if (set.frames.empty()) bad_option("route", "goal_keyframe", "names a key-frame of an empty set");
    const int64_t k = ropt.goal_keyframe, i = k < 0 ? (int64_t)set.frames.size() - 1 : k;
    if (i >= (int64_t)set.frames.size()) bad_option("route", "goal_keyframe", "is " + std::to_string(k) + ", the set has " + std::to_string(set.frames.size()) + " key-frames");
    ropt.goal_x = set.frames[(size_t)i].pose[3];
    ropt.goal_y = set.frames[(size_t)i].pose[7];
    if (!std::isfinite(ropt.goal_x) || !std::isfinite(ropt.goal_y)) bad_option("route", "goal_keyframe", "names a key-frame whose pose is not finite");
  }
  std::vector<Pose12> poses(set.frames.size());
  for (size_t k = 0; k < set.frames.size(); k++) std::copy(set.frames[k].pose, set.frames[k].pose + 12, poses[k].begin());
  // the source map and the base as build_costmap_from_keyframes
  CostmapBase base;
  if (copt.source == "traversability") {
    const TraversabilityOptions topt = TraversabilityOptions::FromConfig(pipeline);
    copt.maxCells(topt.resolution);
    if (!ctx) ctx = DeviceContext::Default();
    base = costmap_base(build_traversability_map(set, topt, ctx));
  } else {
    const OccupancyGridOptions gopt = OccupancyGridOptions::FromConfig(pipeline);
    copt.maxCells(gopt.resolution);
    if (!ctx) ctx = DeviceContext::Default();
    base = costmap_base(build_occupancy_grid(set, gopt, ctx));
  }
  RoutePlanner planner(std::move(base), std::move(poses), copt, ropt, ctx);
  ReplanRun run;
  for (const ReplanEvent& e : events) {
    ReplanEventResult res;
    res.event = e;
    if (e.verb == ReplanEvent::kAt) {
      res.route = (int64_t)run.routes.size();
      run.routes.push_back(planner.routeFrom(e.v[0], e.v[1]));
      run.route_costmaps.push_back(planner.costmap());
    } else {
      CellRect r;
      try {
        r = replan_metre_rect(planner.costmap(), e.v[0], e.v[1], e.v[2], e.v[3]);
      } catch (const std::runtime_error&) {
        bad_line(e.line, "a corner of the rectangle has no cell index");
      }
      res.update.rect = r;
      if (r.empty) run.rects_outside++;
      else res.update = planner.fill(r, e.verb == ReplanEvent::kBlock ? (uint8_t)MH_NAV_LETHAL : (uint8_t)0);
    }
    run.events.push_back(res);
  }
  run.costmap = planner.costmap();
  return run;
}

void write_replan_routes(const ReplanRun& run, const std::string& prefix) {
  if (run.routes.size() != run.route_costmaps.size()) throw std::runtime_error("write_replan_routes: the run's routes and their costmaps differ in number");
  for (size_t k = 0; k < run.routes.size(); k++) write_route(run.routes[k], run.route_costmaps[k], prefix, "_route_" + std::to_string(k));
}

std::string replan_event_summary(const ReplanRun& run, size_t k) {
  const ReplanEventResult& e = run.events.at(k);
  char buf[640];
  if (e.event.verb == ReplanEvent::kAt) {
    const RoutePlan& r = run.routes.at((size_t)e.route);
    snprintf(buf, sizeof buf,
             "{\"event\": %zu, \"line\": %u, \"verb\": \"at\", \"route\": %lld, \"status\": \"%s\", \"cells\": %zu, \"length_m\": %.9g, \"cost_to_go\": %u, "
             "\"max_cost\": %u, \"min_clearance_m\": %.9g, \"seconds_trace\": %.6f}",
             k, e.event.line, (long long)e.route, r.status.c_str(), r.cells.size() / 2, r.length_m, r.cost_to_go, r.max_cost, r.min_clearance_m, r.seconds_trace);
  } else {
    const ReplanUpdate& u = e.update;
    snprintf(buf, sizeof buf,
             "{\"event\": %zu, \"line\": %u, \"verb\": \"%s\", \"cells\": [%u, %u, %u, %u], \"outside\": %s, \"grown\": [%u, %u, %u, %u], \"cells_changed\": %llu, "
             "\"cells_repriced\": %llu, \"withdrawn\": %llu, \"withdraw_sweeps\": %u, \"relax_sweeps\": %u, \"tile_runs_withdraw\": %llu, \"tile_runs_relax\": %llu, "
             "\"seconds_inflate\": %.6f, \"seconds_update\": %.6f}",
             k, e.event.line, e.event.verbName(), u.rect.col0, u.rect.row0, u.rect.w, u.rect.h, u.rect.empty ? "true" : "false", u.grown.col0, u.grown.row0,
             u.grown.w, u.grown.h, (unsigned long long)u.info.n_cells_changed, (unsigned long long)u.info.n_cells_repriced,
             (unsigned long long)u.info.n_withdrawn, u.info.n_withdraw_sweeps, u.info.n_relax_sweeps, (unsigned long long)u.info.n_tile_runs_withdraw,
             (unsigned long long)u.info.n_tile_runs_relax, u.seconds_inflate, u.seconds_update);
  }
  return buf;
}

}  // namespace mola_hip
