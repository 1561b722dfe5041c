// plan_host_check.cpp -- the host rules of mola_lidar_odometry_hip/RoutePlan.h in a stand-alone program, meant to be built with
// -fsanitize=address,undefined (tools/plan_host_check.sh).  No device is asked for: the route: options and their refusals, the price
// table against a restatement formed here, the wrap-around bound at its edge, the cell rule, the summary on random walks, the files
// against bytes formed here, a costmap written and read back under a route, and the statuses plan_route settles before a device.
// Exit status 0 and "ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>

#include "mola_lidar_odometry_hip/RoutePlan.h"

using namespace mola_hip;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static std::string slurp(const std::string& path) {
  std::ifstream in(path, std::ios::binary);
  std::stringstream ss;
  ss << in.rdbuf();
  return ss.str();
}

template <class F>
static bool refuses(F&& f, const char* naming = "") {
  try {
    f();
  } catch (const std::runtime_error& e) {
    return std::string(e.what()).find(naming) != std::string::npos;
  }
  return false;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  std::mt19937 rng(16);
  // ---- options
  auto from = [](const std::string& text) { return RouteOptions::FromConfig(mp2p_icp_hip::Config::FromYamlText(text)); };
  const RouteOptions d = from("");
  CHECK(!d.hasStart() && !d.hasGoal() && d.start_keyframe == 0 && d.goal_keyframe == -1 && d.neutral_price == 4 && d.cost_factor == 0.08);
  CHECK(d.max_route_cells == 1048576);
  const RouteOptions o = from("route:\n  start_x: -1.5\n  start_y: 2\n  goal_x: 30\n  goal_y: 0.25\n  start_keyframe: 2\n  goal_keyframe: 5\n  neutral_price: 1\n"
                              "  cost_factor: 1.5\n  max_route_cells: 7\n");
  CHECK(o.hasStart() && o.hasGoal() && o.start_x == -1.5 && o.start_y == 2.0 && o.goal_x == 30.0 && o.goal_y == 0.25 && o.start_keyframe == 2);
  CHECK(o.goal_keyframe == 5 && o.neutral_price == 1 && o.cost_factor == 1.5 && o.max_route_cells == 7);
  CHECK(from("route:\n").neutral_price == 4 && from("costmap:\n  inscribed_radius: 1\n").cost_factor == 0.08);
  for (const char* bad : {"route:\n  no_such_key: 1\n", "route:\n  start_x: 1\n", "route:\n  start_y: 1\n", "route:\n  goal_x: 1\n", "route:\n  goal_y: 1\n",
                          "route:\n  start_x: nan\n  start_y: 0\n", "route:\n  goal_x: 0\n  goal_y: inf\n", "route:\n  start_keyframe: -2\n",
                          "route:\n  goal_keyframe: 0.5\n", "route:\n  neutral_price: 0\n", "route:\n  neutral_price: -3\n", "route:\n  neutral_price: 2.5\n",
                          "route:\n  cost_factor: -1\n", "route:\n  cost_factor: nan\n", "route:\n  cost_factor: much\n", "route:\n  max_route_cells: 0\n",
                          "route:\n  max_route_cells: [3]\n", "route:\n  max_route_cells: 5000000000\n"})
    CHECK(refuses([&] { (void)from(bad); }, "route: "));
  // ---- the price table
  for (uint32_t np : {1u, 4u, 300u, 65535u})
    for (double cf : {0.0, 0.08, 0.0625, 1.0, 3.9999, 259.0}) {
      RouteOptions opt;
      opt.neutral_price = np;
      opt.cost_factor = cf;
      const double top = (double)np + std::floor(cf * 252.0);
      if (top > 65535.0) {
        CHECK(refuses([&] { (void)route_price_table(opt); }, "65535"));
        continue;
      }
      const std::vector<uint16_t> t = route_price_table(opt);
      CHECK(t.size() == kCostmapPassableBelow);
      for (uint32_t c = 0; c < t.size(); c++) CHECK((double)t[c] == (double)np + std::floor(cf * (double)c) && t[c] >= 1);
    }
  // ---- the wrap-around bound: (n - 1) * 14 * max(price) < 2^32 - 1
  CHECK(!refuses([&] { route_check_window(std::vector<uint16_t>(253, 18), 1ull << 24); }));
  CHECK(refuses([&] { route_check_window(std::vector<uint16_t>(253, 19), 1ull << 24); }, "16146494 cells"));  // 4294967294 / 266 + 1
  CHECK(!refuses([&] { route_check_window({1, 306, 2}, 1000000); }) && refuses([&] { route_check_window({1, 307, 2}, 1000000); }, "route: "));
  CHECK(!refuses([&] { route_check_window({65535}, 4682); }) && refuses([&] { route_check_window({65535}, 4683); }, "4682 cells"));
  CHECK(!refuses([&] { route_check_window({1}, 1ull << 26); }) && refuses([&] { route_check_window({}, 5); }) && refuses([&] { route_check_window({1}, 0); }));
  // ---- the cell rule
  NavCostmap win;
  win.x0 = -5; win.y0 = -3; win.nx = 12; win.ny = 9;
  win.resolution = 0.2;
  win.cost.assign(108, 0);
  win.reach.assign(108, 0);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  struct P { double x, y; int32_t col, row; };
  for (const P& p : {P{0, 0, 5, 3}, P{-0.01, -0.01, 4, 2}, P{1.39, 1.19, 11, 8}, P{1.41, 0, -1, -1}, P{0, -0.61, -1, -1}, P{nan, 0, -1, -1}, P{0, inf, -1, -1},
                     P{3.0e5, 0, -1, -1}, P{-1.0, -0.6, 0, 0}, P{1.0e30, 1.0e30, -1, -1}}) {
    int32_t col = 7, row = 7;
    CHECK(route_cell(win, p.x, p.y, col, row) == (p.col >= 0) && col == p.col && row == p.row);
  }
  // ---- the summary and the files on random walks
  for (int round = 0; round < 20; round++) {
    NavCostmap c;
    c.x0 = -7; c.y0 = 3; c.nx = 2 + rng() % 23; c.ny = 2 + rng() % 11;
    c.resolution = 0.25; c.inscribed_radius = 0.3; c.inflation_radius = 0.8;
    const size_t n = (size_t)c.nx * c.ny;
    c.cost.resize(n); c.reach.assign(n, 0);
    if (round % 3) c.d2.resize(n);
    for (size_t i = 0; i < n; i++) {
      const uint32_t k = rng() % 8;
      c.cost[i] = k == 0 ? 255 : k == 1 ? 254 : k == 2 ? 253 : (uint8_t)(rng() % 253);
      if (!c.d2.empty()) c.d2[i] = rng() % 2 ? (uint16_t)MH_NAV_FAR : (uint16_t)(1 + rng() % 17);
    }
    RoutePlan r;
    int32_t x = (int32_t)(rng() % c.nx), y = (int32_t)(rng() % c.ny);
    const size_t steps = round == 0 ? 0 : rng() % 40;
    double length = 0;
    uint32_t top = 0, near = MH_NAV_FAR;
    std::string txt, tri = "P5\n" + std::to_string(c.nx) + " " + std::to_string(c.ny) + "\n255\n";
    std::vector<uint8_t> on(n, 0);
    for (size_t k = 0; k <= steps; k++) {
      if (k > 0) {
        int32_t u, v;
        do {
          u = x + (int32_t)(rng() % 3) - 1;
          v = y + (int32_t)(rng() % 3) - 1;
        } while ((u == x && v == y) || u < 0 || v < 0 || u >= (int32_t)c.nx || v >= (int32_t)c.ny);
        length += (u != x && v != y) ? 0.25 * std::sqrt(2.0) : 0.25;
        x = u; y = v;
      }
      r.cells.push_back(x);
      r.cells.push_back(y);
      const size_t i = (size_t)y * c.nx + (size_t)x;
      on[i] = 1;
      top = std::max<uint32_t>(top, c.cost[i]);
      if (!c.d2.empty()) near = std::min<uint32_t>(near, c.d2[i]);
      char line[64];
      snprintf(line, sizeof line, "%.9g %.9g\n", (-7 + x + 0.5) * 0.25, (3 + y + 0.5) * 0.25);
      txt += line;
    }
    route_summarise(r, c);
    CHECK(r.xy.size() == r.cells.size() && r.length_m == length && r.max_cost == top);
    CHECK(near == MH_NAV_FAR ? r.min_clearance_m == -1.0 : r.min_clearance_m == std::sqrt((double)near) * 0.25);
    for (uint32_t row = 0; row < c.ny; row++)
      for (uint32_t col = 0; col < c.nx; col++) {
        const size_t i = (size_t)(c.ny - 1 - row) * c.nx + col;
        tri += (char)(on[i] ? 100 : c.cost[i] == 255 ? 205 : c.cost[i] >= 253 ? 0 : 254);
      }
    const std::string prefix = dir + "/r" + std::to_string(round);
    write_route(r, c, prefix);
    CHECK(slurp(prefix + "_route.txt") == txt && slurp(prefix + "_route.pgm") == tri);
    // the costmap under the route through its own files: the reader gives back what the planner's command line starts from
    write_costmap(c, prefix);
    const NavCostmap back = read_costmap(prefix);
    CHECK(back.cost == c.cost && back.d2.empty() && back.nx == c.nx && back.ny == c.ny && back.x0 == c.x0 && back.y0 == c.y0);
    RoutePlan again;
    again.cells = r.cells;
    route_summarise(again, back);
    CHECK(again.xy == r.xy && again.length_m == r.length_m && again.max_cost == r.max_cost && again.min_clearance_m == -1.0);
    write_route(again, back, prefix + "b");
    CHECK(slurp(prefix + "b_route.txt") == txt && slurp(prefix + "b_route.pgm") == tri);
    if (round == 1) {  // refusals
      CHECK(refuses([&] { write_route(r, c, dir + "/no_such_dir/r"); }));
      RoutePlan bad = r;
      bad.cells.push_back(0);
      CHECK(refuses([&] { route_summarise(bad, c); }));
      bad = r;
      bad.cells[0] = (int32_t)c.nx;
      CHECK(refuses([&] { route_summarise(bad, c); }) && refuses([&] { write_route(bad, c, prefix + "x"); }));
      bad = r;
      bad.cells.push_back(bad.cells[bad.cells.size() - 2]);
      bad.cells.push_back(bad.cells[bad.cells.size() - 2]);  // the last cell twice: no step
      CHECK(refuses([&] { route_summarise(bad, c); }));
      bad = r;
      bad.xy.pop_back();
      CHECK(refuses([&] { write_route(bad, c, prefix + "x"); }));
      NavCostmap short_c = c;
      short_c.cost.pop_back();
      CHECK(refuses([&] { route_summarise(r, short_c); }) && refuses([&] { write_route(r, short_c, prefix + "x"); }));
    }
  }
  // ---- what plan_route settles before a device is asked for
  {
    NavCostmap c = win;
    c.cost[3 * 12 + 5] = 254;
    c.cost[4 * 12 + 6] = 253;
    auto at = [&](int col, int row, double& x, double& y) { x = (-5 + col + 0.5) * 0.2; y = (-3 + row + 0.5) * 0.2; };
    struct Q { int sc, sr, gc, gr; const char* status; };
    for (const Q& q : {Q{40, 1, 1, 1, "start_outside"}, Q{5, 3, 1, 1, "start_blocked"}, Q{1, 1, -9, 1, "goal_outside"}, Q{1, 1, 6, 4, "goal_blocked"},
                       Q{5, 3, 40, 1, "start_blocked"}}) {
      RouteOptions opt;
      at(q.sc, q.sr, opt.start_x, opt.start_y);
      at(q.gc, q.gr, opt.goal_x, opt.goal_y);
      const RoutePlan r = plan_route(c, opt);
      CHECK(r.status == q.status && r.cells.empty() && r.field.empty() && r.cost_to_go == MH_PLAN_UNREACHED && r.length_m == 0 && r.min_clearance_m == -1.0);
    }
    RouteOptions none;
    CHECK(refuses([&] { (void)plan_route(c, none); }, "route: start_x"));
    at(1, 1, none.start_x, none.start_y);
    CHECK(refuses([&] { (void)plan_route(c, none); }, "route: goal_x"));
    at(2, 2, none.goal_x, none.goal_y);
    none.neutral_price = 65535;
    none.cost_factor = 1;
    CHECK(refuses([&] { (void)plan_route(c, none); }, "65535"));
    none.cost_factor = 0;
    NavCostmap big = c;
    big.nx = 100; big.ny = 100;
    big.cost.assign(10000, 0);
    CHECK(refuses([&] { (void)plan_route(big, none); }, "4682 cells"));  // prices of 65535 admit 4682 cells
  }
  printf("ok\n");
  return 0;
}
