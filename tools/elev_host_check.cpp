// elev_host_check.cpp -- the host rules of mola_lidar_odometry_hip/Traversability.h in a stand-alone program, meant to be built with
// -fsanitize=address,undefined (tools/elev_host_check.sh).  No device is asked for: the traversability: options and their refusals,
// the derived integers, the cost rule on random planes against a restatement formed here, the four files against bytes formed
// here, the reader's round trip and its refusals.  Exit status 0 and "ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>

#include "mola_lidar_odometry_hip/OccupancyGrid.h"
#include "mola_lidar_odometry_hip/Traversability.h"

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

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  std::mt19937 rng(14);
  // ---- options
  auto from = [](const char* text) { return TraversabilityOptions::FromConfig(mp2p_icp_hip::Config::FromYamlText(text)); };
  const TraversabilityOptions d = from("");
  CHECK(d.resolution == 0.20 && d.z_quantum == 0.01 && d.max_range == 0.0 && d.vehicle_height == 2.0 && d.max_step == 0.15);
  CHECK(d.slope_radius_cells == 2 && d.max_slope_deg == 20.0 && d.min_points_per_cell == 2 && d.min_obstacle_points == 2);
  CHECK(d.target_map.empty() && d.margin_cells == 2);
  CHECK(d.clearanceQ() == 200 && d.stepQ() == 15 && d.riseQ() == 14);
  const TraversabilityOptions o = from("traversability:\n  resolution: 0.25\n  z_quantum: 0.02\n  slope_radius_cells: 4\n  max_slope_deg: 30\n"
                                       "  target_map: points\n  margin_cells: 0\n  min_points_per_cell: 1\n");
  CHECK(o.resolution == 0.25 && o.z_quantum == 0.02 && o.slope_radius_cells == 4 && o.target_map == "points" && o.margin_cells == 0);
  CHECK(o.riseQ() == (int32_t)std::floor(std::tan(30.0 * 3.14159265358979323846 / 180.0) * 4 * 0.25 / 0.02) && o.clearanceQ() == 100);
  for (const char* bad : {"traversability:\n  no_such_key: 1\n", "traversability:\n  resolution: 0\n", "traversability:\n  z_quantum: -1\n",
                          "traversability:\n  max_range: -1\n", "traversability:\n  vehicle_height: 0\n", "traversability:\n  vehicle_height: 1e9\n",
                          "traversability:\n  max_step: -0.1\n", "traversability:\n  slope_radius_cells: 0\n", "traversability:\n  slope_radius_cells: 5\n",
                          "traversability:\n  max_slope_deg: 90\n", "traversability:\n  max_slope_deg: nan\n", "traversability:\n  min_points_per_cell: 0\n",
                          "traversability:\n  min_obstacle_points: 0\n", "traversability:\n  margin_cells: 1.5\n", "traversability:\n  resolution: wide\n"})
    CHECK(refuses([&] { (void)from(bad); }));
  // ---- the cost rule and the files
  for (int trial = 0; trial < 50; trial++) {
    TraversabilityMap m;
    m.nx = 1 + rng() % 40;
    m.ny = 1 + rng() % 40;
    m.step_q = (int32_t)(rng() % 20);
    m.rise_q = (int32_t)(rng() % 20);
    m.min_points_per_cell = 1 + rng() % 3;
    m.min_obstacle_points = 1 + rng() % 3;
    m.z_quantum = trial % 2 ? 0.01 : 0.05;
    m.resolution = trial % 3 ? 0.2 : 0.25;
    m.x0 = (int32_t)(rng() % 400) - 200;
    m.y0 = (int32_t)(rng() % 400) - 200;
    const size_t n = (size_t)m.nx * m.ny;
    m.ground.resize(n); m.count.resize(n); m.obstacle_count.resize(n); m.relief1.resize(n); m.reliefR.resize(n); m.top.resize(n);
    for (size_t i = 0; i < n; i++) {
      m.count[i] = rng() % 5;
      m.obstacle_count[i] = rng() % 4;
      m.ground[i] = m.count[i] ? (int32_t)(rng() % 10000) - 5000 : INT32_MAX;
      const bool known = m.count[i] >= m.min_points_per_cell;
      m.relief1[i] = known ? (int32_t)(rng() % 30) : MH_ELEV_NONE;
      m.reliefR[i] = known ? (int32_t)(rng() % 30) : MH_ELEV_NONE;
    }
    traversability_classify(m);
    uint64_t cnt[3] = {0, 0, 0};
    for (size_t i = 0; i < n; i++) {
      uint8_t want;
      if (m.count[i] < m.min_points_per_cell) want = kCostUnknown;
      else if (m.obstacle_count[i] >= m.min_obstacle_points || m.relief1[i] > m.step_q || m.reliefR[i] > m.rise_q) want = kCostLethal;
      else want = (uint8_t)std::max(252 * m.relief1[i] / (m.step_q + 1), 252 * m.reliefR[i] / (m.rise_q + 1));
      CHECK(m.cost[i] == want);
      CHECK(want == kCostUnknown ? std::isnan(m.height[i]) : m.height[i] == (float)((double)m.ground[i] * m.z_quantum));
      CHECK(want >= kCostLethal || want < 252);
      cnt[want == kCostLethal ? 0 : want == kCostUnknown ? 2 : 1]++;
    }
    CHECK(m.cells_lethal == cnt[0] && m.cells_free == cnt[1] && m.cells_unknown == cnt[2]);
    const std::string name = "map" + std::to_string(trial), prefix = dir + "/" + name;
    write_traversability_map(m, prefix);
    std::string pgm = "P5\n" + std::to_string(m.nx) + " " + std::to_string(m.ny) + "\n255\n", cost = pgm, f32;
    for (uint32_t r = 0; r < m.ny; r++)
      for (uint32_t c = 0; c < m.nx; c++) {
        const uint8_t v = m.cost[(size_t)(m.ny - 1 - r) * m.nx + c];
        pgm.push_back((char)(v == kCostLethal ? 0 : v == kCostUnknown ? 205 : 254));
        cost.push_back((char)v);
      }
    for (size_t i = 0; i < n; i++) {
      char b[4];
      memcpy(b, &m.height[i], 4);  // (this program runs on little-endian hosts)
      f32.append(b, 4);
    }
    CHECK(slurp(prefix + ".pgm") == pgm && slurp(prefix + "_cost.pgm") == cost && slurp(prefix + "_height.f32") == f32);
    char yaml[768];
    snprintf(yaml, sizeof(yaml), "image: %s.pgm\nresolution: %.9g\norigin: [%.9g, %.9g, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
             "cost_image: %s_cost.pgm\nheight_file: %s_height.f32\nz_quantum: %.9g\nheight_row_order: bottom_up\n",
             name.c_str(), m.resolution, m.x0 * m.resolution, m.y0 * m.resolution, name.c_str(), name.c_str(), m.z_quantum);
    CHECK(slurp(prefix + ".yaml") == yaml);
    const TraversabilityMap back = read_traversability_map(prefix);
    CHECK(back.x0 == m.x0 && back.y0 == m.y0 && back.nx == m.nx && back.ny == m.ny && back.resolution == m.resolution && back.z_quantum == m.z_quantum);
    CHECK(back.cost == m.cost && memcmp(back.height.data(), m.height.data(), 4 * n) == 0);
    CHECK(back.cells_lethal == cnt[0] && back.cells_free == cnt[1] && back.cells_unknown == cnt[2] && back.ground.empty());
    const OccupancyGrid g = read_occupancy_grid(prefix);  // the trinary pair is g12's
    CHECK(g.nx == m.nx && g.ny == m.ny && g.cells_occupied == cnt[0] && g.cells_free == cnt[1] && g.cells_unknown == cnt[2]);
    if (trial == 0) {  // truncated files, a foreign byte, a missing file, an unwritable place, planes of the wrong size
      spit(prefix + "_height.f32", f32.substr(0, f32.size() - 1));
      CHECK(refuses([&] { (void)read_traversability_map(prefix); }));
      spit(prefix + "_height.f32", f32);
      spit(prefix + "_cost.pgm", cost.substr(0, cost.size() - 1));
      CHECK(refuses([&] { (void)read_traversability_map(prefix); }));
      std::string other = cost;
      other.back() = (char)((uint8_t)other.back() == kCostLethal ? 0 : kCostLethal);
      spit(prefix + "_cost.pgm", other);
      CHECK(refuses([&] { (void)read_traversability_map(prefix); }));
      other.back() = (char)253;
      spit(prefix + "_cost.pgm", other);
      CHECK(refuses([&] { (void)read_traversability_map(prefix); }));
      spit(prefix + "_cost.pgm", cost);
      (void)read_traversability_map(prefix);
      CHECK(refuses([&] { (void)read_traversability_map(dir + "/nowhere"); }));
      CHECK(refuses([&] { write_traversability_map(m, dir + "/no_such_dir/map"); }));
      TraversabilityMap empty;
      CHECK(refuses([&] { write_traversability_map(empty, prefix); }));
      TraversabilityMap wrong = m;
      wrong.reliefR.pop_back();
      CHECK(refuses([&] { traversability_classify(wrong); }));
      OccupancyGrid plain;
      plain.nx = plain.ny = 2;
      plain.resolution = 0.2;
      plain.cells.assign(4, kGridFree);
      write_occupancy_grid(plain, dir + "/plain");
      CHECK(refuses([&] { (void)read_traversability_map(dir + "/plain"); }));
    }
  }
  // ---- a cost image whose first pixels (the largest y, from column 0) are white space to a careless header parser reads back
  for (int first : {9, 10, 11, 12, 13, 32, -1}) {
    TraversabilityMap m;
    m.nx = 4; m.ny = 3;
    m.resolution = 0.2; m.z_quantum = 0.01;
    m.x0 = -7; m.y0 = 3;
    m.cost = {255, 0, 17, 254, 251, 254, 255, 1, 0, 0, 0, 0};
    if (first >= 0) m.cost[8] = (uint8_t)first;
    else { m.cost[8] = 10; m.cost[9] = 32; m.cost[10] = 9; }
    m.height.assign(12, 0.25f);
    const std::string prefix = dir + "/white" + std::to_string(first + 1);
    write_traversability_map(m, prefix);
    const std::string cost = slurp(prefix + "_cost.pgm");
    CHECK(cost.size() == 11 + 12 && cost.compare(0, 11, "P5\n4 3\n255\n") == 0 && (uint8_t)cost[11] == m.cost[8]);
    const TraversabilityMap back = read_traversability_map(prefix);
    CHECK(back.nx == 4 && back.ny == 3 && back.cost == m.cost && back.height == m.height);
    CHECK(back.cells_lethal == 2 && back.cells_free == 8 && back.cells_unknown == 2);
    for (const char* head : {"P5\n4 3\n255 ", "P5\n4 3\n255\n\n", "P5\n4 3\n254\n", "P5\n3 4\n255\n", "P5\n4 4\n255\n"}) {  // not the writer's header
      spit(prefix + "_cost.pgm", head + cost.substr(11));
      CHECK(refuses([&] { (void)read_traversability_map(prefix); }));
    }
  }
  // ---- a set without points is refused before any device is asked for
  molahip_host::KeyFrameSet set;
  CHECK(refuses([&] { (void)build_traversability_map(set, d); }));
  set.maps.resize(1);
  set.maps[0].name = "localmap";
  set.maps[0].class_name = "HashedVoxelPointCloud";
  set.frames.resize(3);
  CHECK(refuses([&] { (void)build_traversability_map(set, d); }));
  TraversabilityOptions other = d;
  other.target_map = "elsewhere";
  CHECK(refuses([&] { (void)build_traversability_map(set, other); }));
  printf("ok\n");
  return 0;
}
