// replan_host_check.cpp -- the host rules of mola_lidar_odometry_hip/Replan.h in a stand-alone program, meant to be built with
// -fsanitize=address,undefined (tools/replan_host_check.sh).  No device is asked for: the events reader on good, malformed and
// truncated texts and files, the metre rectangle and the grown rectangle against restatements formed here, the route files per `at`
// event against bytes formed here, the summaries, and what a RoutePlanner refuses before a device.
// Exit status 0 and "ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>

#include "mola_lidar_odometry_hip/Replan.h"

using namespace mola_hip;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static std::string slurp_file(const std::string& path) {
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
  std::mt19937 rng(17);
  // ---- the events text
  const std::string good = "# a lorry parks across the road\nblock 1 2 3.5 -4e0   # trailing comment\n\nat 0.5 0.25\nclear 1 2 3.5 -4\n  at\t-1 +2\n";
  {
    const std::vector<ReplanEvent> e = parse_replan_events(good);
    CHECK(e.size() == 4 && e[0].verb == ReplanEvent::kBlock && e[0].line == 2 && e[0].v[0] == 1 && e[0].v[1] == 2 && e[0].v[2] == 3.5 && e[0].v[3] == -4);
    CHECK(e[1].verb == ReplanEvent::kAt && e[1].line == 4 && e[1].v[0] == 0.5 && e[1].v[1] == 0.25);
    CHECK(e[2].verb == ReplanEvent::kClear && e[2].line == 5 && e[3].verb == ReplanEvent::kAt && e[3].line == 6 && e[3].v[0] == -1 && e[3].v[1] == 2);
    CHECK(std::string(e[0].verbName()) == "block" && std::string(e[2].verbName()) == "clear" && std::string(e[3].verbName()) == "at");
    CHECK(parse_replan_events("").empty() && parse_replan_events("# nothing\n\n").empty() && parse_replan_events("\n\n\n").empty());
    CHECK(parse_replan_events("at 1 2").size() == 1 && parse_replan_events("at 1 2\r\n").size() == 1);
  }
  struct B { const char* text; const char* naming; };
  for (const B& b : {B{"block 1 2 3", "events: line 1"}, B{"at 1", "events: line 1"}, B{"at 1 2 3", "events: line 1"}, B{"\nmove 1 2", "events: line 2"},
                     B{"at 1 two", "events: line 1"}, B{"block 1 2 3 nan", "events: line 1"}, B{"at inf 0", "events: line 1"}, B{"at 0x10 0", "events: line 1"},
                     B{"at 1 2\nblock", "events: line 2"}, B{"at 1 2\nclear 1 2 3 4 5", "events: line 2"}, B{"BLOCK 1 2 3 4", "events: line 1"},
                     B{"at 1e999 0", "events: line 1"}, B{"at 1 2\n\n\nat 1_0 2", "events: line 4"}, B{"at 1 2,", "events: line 1"}, B{"at - 2", "events: line 1"}})
    CHECK(refuses([&] { (void)parse_replan_events(b.text); }, b.naming));
  // every prefix of a good text either parses or is refused naming a line: a file cut off anywhere
  for (size_t n = 0; n <= good.size(); n++) {
    const std::string cut = good.substr(0, n);
    bool ok = true;
    try {
      (void)parse_replan_events(cut);
    } catch (const std::runtime_error& e) {
      ok = std::string(e.what()).find("events: line ") == 0;
    }
    CHECK(ok);
  }
  // random bytes never do worse than a refusal
  for (int round = 0; round < 300; round++) {
    std::string junk(rng() % 60, ' ');
    for (char& c : junk) c = "blockearat 0123456789.-+e#\n\t\0x"[rng() % 31];
    try {
      (void)parse_replan_events(junk);
    } catch (const std::runtime_error&) {
    }
  }
  // ... from files
  {
    std::ofstream(dir + "/events.txt", std::ios::binary) << good;
    CHECK(read_replan_events(dir + "/events.txt").size() == 4);
    std::ofstream(dir + "/cut.txt", std::ios::binary) << good.substr(0, 40);
    CHECK(refuses([&] { (void)read_replan_events(dir + "/cut.txt"); }, "events: line 2"));
    std::ofstream(dir + "/empty.txt", std::ios::binary) << "";
    CHECK(read_replan_events(dir + "/empty.txt").empty());
    CHECK(refuses([&] { (void)read_replan_events(dir + "/no_such_file.txt"); }, "no_such_file"));
  }
  // ---- the metre rectangle
  NavCostmap win;
  win.x0 = -5; win.y0 = -3; win.nx = 12; win.ny = 9;
  win.resolution = 0.2;
  {
    struct Q { double xa, ya, xb, yb; int col0, row0, w, h; };
    for (const Q& q : {Q{0, 0, 0.39, 0.19, 5, 3, 2, 1}, Q{0.39, 0.19, 0, 0, 5, 3, 2, 1}, Q{-0.01, -0.01, -0.01, -0.01, 4, 2, 1, 1}, Q{-100, -100, 100, 100, 0, 0, 12, 9},
                       Q{1.3, 1.1, 50, 50, 11, 8, 1, 1}, Q{1.41, 0, 50, 1, -1, 0, 0, 0}, Q{0, -9, 1, -0.61, -1, 0, 0, 0}}) {
      const CellRect r = replan_metre_rect(win, q.xa, q.ya, q.xb, q.yb);
      if (q.col0 < 0) CHECK(r.empty);
      else CHECK(!r.empty && (int)r.col0 == q.col0 && (int)r.row0 == q.row0 && (int)r.w == q.w && (int)r.h == q.h);
    }
    CHECK(refuses([&] { (void)replan_metre_rect(win, 0, 0, 3.0e5, 0); }, "cell index") && refuses([&] { (void)replan_metre_rect(win, 0, -1.0e30, 1, 0); }));
    NavCostmap none;
    CHECK(refuses([&] { (void)replan_metre_rect(none, 0, 0, 1, 1); }));
    std::uniform_real_distribution<double> u(-3.0, 3.0);
    for (int round = 0; round < 500; round++) {  // against route_cell on both corners
      const double xa = u(rng), ya = u(rng), xb = u(rng), yb = u(rng);
      const CellRect r = replan_metre_rect(win, xa, ya, xb, yb);
      int32_t c0, r0, c1, r1;
      const bool in_a = route_cell(win, std::min(xa, xb), std::min(ya, yb), c0, r0), in_b = route_cell(win, std::max(xa, xb), std::max(ya, yb), c1, r1);
      if (in_a && in_b) CHECK(!r.empty && (int32_t)r.col0 == c0 && (int32_t)r.row0 == r0 && (int32_t)(r.col0 + r.w - 1) == c1 && (int32_t)(r.row0 + r.h - 1) == r1);
      if (!r.empty) CHECK(r.w >= 1 && r.h >= 1 && r.col0 + r.w <= win.nx && r.row0 + r.h <= win.ny);
    }
  }
  // ---- the grown rectangle
  for (int round = 0; round < 2000; round++) {
    const uint32_t nx = 1 + rng() % 40, ny = 1 + rng() % 40, m = rng() % 4 ? rng() % 8 : 255;
    CellRect r;
    r.empty = false;
    r.col0 = rng() % nx; r.row0 = rng() % ny;
    r.w = 1 + rng() % (nx - r.col0); r.h = 1 + rng() % (ny - r.row0);
    const CellRect g = replan_grown_rect(r, m, nx, ny);
    const long a = std::max<long>((long)r.col0 - m, 0), b = std::max<long>((long)r.row0 - m, 0);
    const long c = std::min<long>((long)r.col0 + r.w + m, nx), d = std::min<long>((long)r.row0 + r.h + m, ny);
    CHECK(!g.empty && g.col0 == a && g.row0 == b && g.w == c - a && g.h == d - b);
  }
  {
    CellRect r;
    CHECK(refuses([&] { (void)replan_grown_rect(r, 3, 10, 10); }));
    r.empty = false;
    r.col0 = 8; r.w = 3; r.h = 1;
    CHECK(refuses([&] { (void)replan_grown_rect(r, 3, 10, 10); }, "leaves the window"));
    r.col0 = 0xFFFFFFFFu; r.w = 2;
    CHECK(refuses([&] { (void)replan_grown_rect(r, 3, 10, 10); }));
    r.col0 = 0; r.w = 0;
    CHECK(refuses([&] { (void)replan_grown_rect(r, 3, 10, 10); }));
  }
  // ---- the route files per `at` event and the summaries, on a run formed here
  {
    ReplanRun run;
    std::vector<std::string> txt, pgm;
    for (int k = 0; k < 3; k++) {
      NavCostmap c = win;
      c.inscribed_radius = 0.3; c.inflation_radius = 0.8;
      c.cost.resize(108); c.reach.assign(108, 0);
      for (auto& v : c.cost) v = rng() % 5 == 0 ? 254 : rng() % 7 == 0 ? 255 : (uint8_t)(rng() % 253);
      RoutePlan r;
      std::string t, img = "P5\n12 9\n255\n";
      std::vector<uint8_t> on(108, 0);
      if (k != 1) {  // (route 1 is empty: an unreachable start writes an empty text and the bare image)
        for (int x = k; x < 9; x++) {
          r.cells.push_back(x);
          r.cells.push_back(k + (x % 2));
          on[(size_t)(k + (x % 2)) * 12 + x] = 1;
          char line[64];
          snprintf(line, sizeof line, "%.9g %.9g\n", (-5 + x + 0.5) * 0.2, (-3 + k + (x % 2) + 0.5) * 0.2);
          t += line;
        }
        r.status = "found";
      } else r.status = "unreachable";
      route_summarise(r, c);
      for (uint32_t row = 0; row < 9; row++)
        for (uint32_t col = 0; col < 12; col++) {
          const size_t i = (size_t)(8 - row) * 12 + col;
          img += (char)(on[i] ? 100 : c.cost[i] == 255 ? 205 : c.cost[i] >= 253 ? 0 : 254);
        }
      txt.push_back(t);
      pgm.push_back(img);
      ReplanEventResult e;
      e.event.verb = ReplanEvent::kAt;
      e.event.line = 1 + 2 * k;
      e.route = k;
      run.events.push_back(e);
      ReplanEventResult b;
      b.event.verb = k % 2 ? ReplanEvent::kClear : ReplanEvent::kBlock;
      b.event.line = 2 + 2 * k;
      if (k < 2) {
        b.update.rect = replan_metre_rect(win, 0, 0, 0.5, 0.5);
        b.update.grown = replan_grown_rect(b.update.rect, 2, 12, 9);
        b.update.info.n_cells_changed = 9;
        b.update.info.n_withdrawn = 4;
      } else run.rects_outside++;
      run.events.push_back(b);
      run.routes.push_back(r);
      run.route_costmaps.push_back(c);
    }
    write_replan_routes(run, dir + "/run");
    for (int k = 0; k < 3; k++) {
      CHECK(slurp_file(dir + "/run_route_" + std::to_string(k) + ".txt") == txt[k]);
      CHECK(slurp_file(dir + "/run_route_" + std::to_string(k) + ".pgm") == pgm[k]);
    }
    CHECK(refuses([&] { write_replan_routes(run, dir + "/no_such_dir/run"); }));
    for (size_t k = 0; k < run.events.size(); k++) {
      const std::string s = replan_event_summary(run, k);
      CHECK(s.front() == '{' && s.back() == '}' && s.find("\"event\": " + std::to_string(k)) != std::string::npos);
      CHECK(s.find(std::string("\"verb\": \"") + run.events[k].event.verbName() + "\"") != std::string::npos);
    }
    CHECK(replan_event_summary(run, 1).find("\"cells\": [5, 3, 3, 3]") != std::string::npos && replan_event_summary(run, 1).find("\"withdrawn\": 4") != std::string::npos);
    CHECK(replan_event_summary(run, 5).find("\"outside\": true") != std::string::npos && replan_event_summary(run, 2).find("\"status\": \"unreachable\"") != std::string::npos);
    bool threw = false;  // (an event that is not there)
    try {
      (void)replan_event_summary(run, 6);
    } catch (const std::exception&) {
      threw = true;
    }
    CHECK(threw);
    run.route_costmaps.pop_back();
    CHECK(refuses([&] { write_replan_routes(run, dir + "/run"); }, "differ in number"));
  }
  // ---- what a RoutePlanner refuses before a device is asked for
  {
    CostmapBase base;
    base.x0 = -5; base.y0 = -3; base.nx = 12; base.ny = 9;
    base.resolution = 0.2;
    base.bytes.assign(108, 0);
    NavCostmapOptions copt;
    RouteOptions ropt;
    CHECK(refuses([&] { RoutePlanner p(base, {}, copt, ropt); }, "route: goal_x"));
    ropt.goal_x = 50; ropt.goal_y = 0;
    CHECK(refuses([&] { RoutePlanner p(base, {}, copt, ropt); }, "outside the window"));
    ropt.goal_x = 0;
    ropt.neutral_price = 65535;
    ropt.cost_factor = 1;
    CHECK(refuses([&] { RoutePlanner p(base, {}, copt, ropt); }, "65535"));
    ropt.cost_factor = 0;
    CostmapBase big = base;
    big.nx = 100; big.ny = 100;
    big.bytes.assign(10000, 0);
    CHECK(refuses([&] { RoutePlanner p(big, {}, copt, ropt); }, "4682 cells"));
    CostmapBase shortb = base;
    shortb.bytes.pop_back();
    CHECK(refuses([&] { RoutePlanner p(shortb, {}, copt, RouteOptions()); }, "ny * nx"));
    copt.inflation_radius = 100;
    ropt = RouteOptions();
    ropt.goal_x = 0; ropt.goal_y = 0;
    CHECK(refuses([&] { RoutePlanner p(base, {}, copt, ropt); }, "costmap: "));
  }
  printf("ok\n");
  return 0;
}
