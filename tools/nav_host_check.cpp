// nav_host_check.cpp -- the host rules of mola_lidar_odometry_hip/NavCostmap.h in a stand-alone program, meant to be built with
// -fsanitize=address,undefined (tools/nav_host_check.sh).  No device is asked for: the costmap: options and their refusals, the
// inflation table against a restatement formed here, the base plane from both kinds of source map, the seeds, the counts on random
// planes, the files against bytes formed here, the reader's round trip and its refusals.  Exit status 0 and "ok" when every check
// holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>

#include "mola_lidar_odometry_hip/NavCostmap.h"

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

static void spit(const std::string& path, const std::string& bytes) {
  std::ofstream out(path, std::ios::binary | std::ios::trunc);
  out.write(bytes.data(), (std::streamsize)bytes.size());
}

template <class F>
static bool refuses(F&& f) {
  try {
    f();
  } catch (const std::runtime_error&) {
    return true;
  }
  return false;
}

static Pose12 pose(double x, double y) { return Pose12{1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, 0}; }

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  std::mt19937 rng(15);
  // ---- options
  auto from = [](const std::string& text) { return NavCostmapOptions::FromConfig(mp2p_icp_hip::Config::FromYamlText(text)); };
  const NavCostmapOptions d = from("");
  CHECK(d.source == "traversability" && d.inscribed_radius == 0.5 && d.inflation_radius == 1.5 && d.cost_scaling == 3.0);
  CHECK(!d.unknown_is_obstacle && d.reach_from == "keyframes");
  const NavCostmapOptions o = from("costmap:\n  source: occupancy_grid\n  inscribed_radius: 0.25\n  inflation_radius: 0.25\n  cost_scaling: 10\n"
                                   "  unknown_is_obstacle: true\n  reach_from: first\n");
  CHECK(o.source == "occupancy_grid" && o.inscribed_radius == 0.25 && o.inflation_radius == 0.25 && o.cost_scaling == 10.0);
  CHECK(o.unknown_is_obstacle && o.reach_from == "first");
  for (const char* bad : {"costmap:\n  no_such_key: 1\n", "costmap:\n  source: points\n", "costmap:\n  inscribed_radius: -1\n",
                          "costmap:\n  inscribed_radius: nan\n", "costmap:\n  inflation_radius: 0.4\n", "costmap:\n  inflation_radius: inf\n",
                          "costmap:\n  cost_scaling: 0\n", "costmap:\n  unknown_is_obstacle: maybe\n", "costmap:\n  reach_from: last\n",
                          "costmap:\n  inscribed_radius: wide\n"})
    CHECK(refuses([&] { (void)from(bad); }));
  CHECK(d.maxCells(0.2) == 8 && d.maxCells(0.05) == 30 && d.maxCells(0.25) == 6);
  CHECK(refuses([&] { (void)from("costmap:\n  inflation_radius: 51.3\n").maxCells(0.2); }));
  CHECK(from("costmap:\n  inflation_radius: 51\n").maxCells(0.2) == 255);
  CHECK(refuses([&] { (void)d.maxCells(0.0); }));
  // ---- the table
  for (double res : {0.05, 0.2, 0.25})
    for (const char* text : {"", "costmap:\n  inscribed_radius: 1\n  inflation_radius: 2\n", "costmap:\n  inscribed_radius: 0.75\n  inflation_radius: 0.75\n",
                             "costmap:\n  inscribed_radius: 0\n  inflation_radius: 0\n", "costmap:\n  inscribed_radius: 2\n  inflation_radius: 12.75\n  cost_scaling: 0.2\n"}) {
      const NavCostmapOptions opt = from(text);
      const std::vector<uint8_t> t = inflation_table(opt, res);
      const uint32_t R = (uint32_t)std::ceil(opt.inflation_radius / res);
      CHECK(R == opt.maxCells(res) && t.size() == (size_t)R * R + 1 && t[0] == 0);
      for (uint32_t d2 = 1; d2 <= R * R; d2++) {
        const double dist = std::sqrt((double)d2) * res;
        const int want = dist <= opt.inscribed_radius ? 253
                         : dist <= opt.inflation_radius ? (int)std::floor(252.0 * std::exp(-opt.cost_scaling * (dist - opt.inscribed_radius))) : 0;
        CHECK(t[d2] == want && t[d2] <= 253);
      }
    }
  // ---- the base plane
  TraversabilityMap tm;
  tm.x0 = -3; tm.y0 = 2; tm.nx = 7; tm.ny = 5;
  tm.resolution = 0.2;
  tm.cost.resize(35);
  for (auto& v : tm.cost) v = (uint8_t)(rng() % 256);
  const CostmapBase tb = costmap_base(tm);
  CHECK(tb.bytes == tm.cost && tb.x0 == -3 && tb.y0 == 2 && tb.nx == 7 && tb.ny == 5 && tb.resolution == 0.2);
  OccupancyGrid og;
  og.nx = 3; og.ny = 2;
  og.resolution = 0.05;
  og.cells = {kGridFree, kGridOccupied, kGridUnknown, kGridUnknown, kGridFree, kGridOccupied};
  CHECK(costmap_base(og).bytes == (std::vector<uint8_t>{0, 254, 255, 255, 0, 254}));
  og.cells[1] = 50;
  CHECK(refuses([&] { (void)costmap_base(og); }));
  tm.nx = 8;
  CHECK(refuses([&] { (void)costmap_base(tm); }));
  // ---- seeds
  CostmapBase win;
  win.x0 = -5; win.y0 = -3; win.nx = 12; win.ny = 9;
  win.resolution = 0.2;
  win.bytes.assign(108, 0);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<Pose12> poses = {pose(0, 0), pose(-0.01, -0.01), pose(1.39, 1.19), pose(1.41, 0), pose(0, -0.61), pose(nan, 0), pose(0, inf),
                                     pose(3.0e5, 0), pose(-1.0, -0.6)};
  CHECK(costmap_seeds(win, poses, "keyframes") == (std::vector<int32_t>{5, 3, 4, 2, 11, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0}));
  CHECK(costmap_seeds(win, poses, "first") == (std::vector<int32_t>{5, 3}) && costmap_seeds(win, poses, "none").empty());
  CHECK(costmap_seeds(win, {}, "first").empty());
  CHECK(refuses([&] { (void)costmap_seeds(win, poses, "all"); }));
  // ---- counts on random planes, the files, the round trip
  for (int round = 0; round < 20; round++) {
    NavCostmap c;
    c.x0 = -7; c.y0 = 3; c.nx = 1 + rng() % 23; c.ny = 1 + rng() % 11;
    c.resolution = 0.25; c.inscribed_radius = 0.3; c.inflation_radius = 0.8;
    const size_t n = (size_t)c.nx * c.ny;
    c.cost.resize(n); c.reach.resize(n); c.d2.resize(n);
    uint64_t want[7] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < n; i++) {
      const uint32_t k = rng() % 8;
      c.cost[i] = k == 0 ? 255 : k == 1 ? 254 : k == 2 ? 253 : (uint8_t)(rng() % 253);
      c.d2[i] = rng() % 2 ? (uint16_t)MH_NAV_FAR : (uint16_t)(rng() % 17);
      c.reach[i] = c.cost[i] < 253 && rng() % 2;
      want[c.cost[i] == 255 ? 0 : c.cost[i] == 254 ? 1 : c.cost[i] == 253 ? 2 : c.d2[i] != MH_NAV_FAR ? 3 : 4]++;
      want[5] += c.reach[i];
      want[6] += c.cost[i] < 253 && !c.reach[i];
    }
    const std::vector<Pose12> kf = {pose(-7 * 0.25 + 0.1, 3 * 0.25 + 0.1), pose(100, 100)};
    costmap_summarise(c, kf);
    CHECK(c.cells_unknown == want[0] && c.cells_lethal == want[1] && c.cells_inscribed == want[2] && c.cells_inflated == want[3]);
    CHECK(c.cells_free == want[4] && c.cells_reached == want[5] && c.cells_unreachable_free == want[6]);
    CHECK(c.keyframe_cost.size() == 2 && c.keyframe_cost[0] == c.cost[0] && c.keyframe_d2[0] == c.d2[0] && c.keyframe_reached[0] == c.reach[0]);
    CHECK(c.keyframe_cost[1] == 255 && c.keyframe_d2[1] == MH_NAV_FAR && c.keyframe_reached[1] == 0);
    CHECK(c.keyframes_blocked == 1u + (c.cost[0] >= 253));
    CHECK(c.d2[0] == MH_NAV_FAR ? c.trajectory_min_clearance_m == -1.0 : c.trajectory_min_clearance_m == std::sqrt((double)c.d2[0]) * 0.25);
    const std::string prefix = dir + "/m" + std::to_string(round);
    write_costmap(c, prefix);
    const std::string head = "P5\n" + std::to_string(c.nx) + " " + std::to_string(c.ny) + "\n255\n";
    std::string tri = head, cost = head, reach = head;
    for (uint32_t r = 0; r < c.ny; r++)
      for (uint32_t x = 0; x < c.nx; x++) {
        const size_t i = (size_t)(c.ny - 1 - r) * c.nx + x;
        tri += (char)(c.cost[i] == 255 ? 205 : c.cost[i] >= 253 ? 0 : 254);
        cost += (char)c.cost[i];
        reach += (char)(c.reach[i] ? 255 : 0);
      }
    CHECK(slurp(prefix + ".pgm") == tri && slurp(prefix + "_cost.pgm") == cost && slurp(prefix + "_reach.pgm") == reach);
    const std::string name = "m" + std::to_string(round);
    CHECK(slurp(prefix + ".yaml") == "image: " + name + ".pgm\nresolution: 0.25\norigin: [-1.75, 0.75, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
                                         "cost_image: " + name + "_cost.pgm\nreach_image: " + name + "_reach.pgm\ninscribed_radius: 0.3\ninflation_radius: 0.8\n");
    const NavCostmap back = read_costmap(prefix);
    CHECK(back.x0 == c.x0 && back.y0 == c.y0 && back.nx == c.nx && back.ny == c.ny && back.resolution == 0.25 && back.cost == c.cost && back.reach == c.reach);
    CHECK(back.d2.empty() && back.inscribed_radius == 0.3 && back.inflation_radius == 0.8 && back.cells_reached == c.cells_reached);
    CHECK(back.cells_lethal == c.cells_lethal && back.cells_inscribed == c.cells_inscribed && back.cells_unknown == c.cells_unknown);
    CHECK(back.cells_unreachable_free == c.cells_unreachable_free && back.cells_inflated == 0 && back.cells_free == 0);
    write_costmap(back, prefix + "b");
    CHECK(slurp(prefix + "b.pgm") == tri && slurp(prefix + "b_cost.pgm") == cost && slurp(prefix + "b_reach.pgm") == reach);
    if (round == 0) {  // the reader's refusals
      CHECK(refuses([&] { (void)read_costmap(dir + "/nowhere"); }));
      CHECK(refuses([&] { write_costmap(c, dir + "/no_such_dir/m"); }));
      NavCostmap bad = c;
      bad.reach.pop_back();
      CHECK(refuses([&] { write_costmap(bad, dir + "/bad"); }));
      CHECK(refuses([&] { costmap_summarise(bad, {}); }));
      std::string cut = cost;
      cut.pop_back();
      spit(prefix + "_cost.pgm", cut);
      CHECK(refuses([&] { (void)read_costmap(prefix); }));
      std::string other = cost;
      other[other.size() - 1] = (char)((unsigned char)other[other.size() - 1] == 255 ? 0 : 255);  // (unknown <-> free: the trinary image disagrees)
      spit(prefix + "_cost.pgm", other);
      CHECK(refuses([&] { (void)read_costmap(prefix); }));
      spit(prefix + "_cost.pgm", cost);
      std::string grey = reach;
      grey[grey.size() - 1] = 7;
      spit(prefix + "_reach.pgm", grey);
      CHECK(refuses([&] { (void)read_costmap(prefix); }));
      spit(prefix + "_reach.pgm", reach);
      const std::string yaml = slurp(prefix + ".yaml");
      spit(prefix + ".yaml", yaml.substr(0, yaml.find("reach_image")));
      CHECK(refuses([&] { (void)read_costmap(prefix); }));
      spit(prefix + ".yaml", yaml);
      (void)read_costmap(prefix);
    }
  }
  printf("ok\n");
  return 0;
}
