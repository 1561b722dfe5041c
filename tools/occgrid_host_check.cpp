// occgrid_host_check.cpp -- the host rules of mola_lidar_odometry_hip/OccupancyGrid.h in a stand-alone program, meant to be built with
// -fsanitize=address,undefined (tools/occgrid_host_check.sh).  No device is asked for: the occupancy_grid: options and their refusals,
// the height-to-index rule, the trinary rule on random maxima, the PGM / YAML writer against bytes formed here, the reader's round
// trip and its refusals.  Exit status 0 and "ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>

#include "mola_lidar_odometry_hip/OccupancyGrid.h"

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
  std::mt19937 rng(12);
  // ---- options
  auto from = [](const char* text) { return OccupancyGridOptions::FromConfig(mp2p_icp_hip::Config::FromYamlText(text)); };
  const OccupancyGridOptions d = from("");
  CHECK(d.resolution == 0.05 && d.prob_hit == 0.70 && d.prob_miss == 0.30 && d.clamp_min == 0.05 && d.clamp_max == 0.95);
  CHECK(d.occupied_threshold == 0.60 && d.ray_trace_free_space && d.max_range == 0.0 && d.decimation == 1 && d.update_rule == "counted");
  CHECK(d.target_map.empty() && d.z_min == -0.10 && d.z_max == 1.50 && d.margin_cells == 2);
  const OccupancyGridOptions o = from("occupancy_grid:\n  resolution: 0.1\n  update_rule: once\n  target_map: points\n  z_min: -1\n  margin_cells: 0\n"
                                      "  ray_trace_free_space: false\n  decimation: 4\n");
  CHECK(o.resolution == 0.1 && o.update_rule == "once" && o.target_map == "points" && o.z_min == -1.0 && o.margin_cells == 0);
  CHECK(!o.ray_trace_free_space && o.decimation == 4);
  for (const char* bad : {"occupancy_grid:\n  no_such_key: 1\n", "occupancy_grid:\n  resolution: 0\n", "occupancy_grid:\n  prob_hit: 1\n",
                          "occupancy_grid:\n  clamp_max: 0.01\n", "occupancy_grid:\n  decimation: 0\n", "occupancy_grid:\n  update_rule: sum\n",
                          "occupancy_grid:\n  z_max: -3\n", "occupancy_grid:\n  z_min: nan\n", "occupancy_grid:\n  margin_cells: 1.5\n",
                          "occupancy_grid:\n  ray_trace_free_space: perhaps\n"})
    CHECK(refuses([&] { (void)from(bad); }));
  // ---- heights to indices
  CHECK(occupancy_grid_z_index(0.0, 0.05) == 0 && occupancy_grid_z_index(-1e-12, 0.05) == -1 && occupancy_grid_z_index(1.0, 0.25) == 4);
  CHECK(occupancy_grid_z_index(-0.10, 0.05) == -2 && occupancy_grid_z_index(1.50, 0.05) == 30);
  std::uniform_real_distribution<double> uz(-50.0, 50.0);
  for (int k = 0; k < 2000; k++) {
    const double z = uz(rng);
    const int32_t i = occupancy_grid_z_index(z, 0.2);
    const double inv = (double)(1.0f / 0.2f);
    CHECK((double)i <= z * inv && z * inv < (double)i + 1.0);
  }
  // ---- the trinary rule
  for (int trial = 0; trial < 50; trial++) {
    OccupancyGrid g;
    g.nx = 1 + rng() % 40;
    g.ny = 1 + rng() % 40;
    g.l_occ = (int32_t)(rng() % 60) - 30;
    g.max_logodds.resize((size_t)g.nx * g.ny);
    for (auto& m : g.max_logodds) m = rng() % 4 == 0 ? MH_OCCGRID_NONE : (int32_t)(rng() % 95) - 47;
    occupancy_grid_classify(g);
    uint64_t n[3] = {0, 0, 0};
    for (size_t i = 0; i < g.cells.size(); i++) {
      const int32_t m = g.max_logodds[i];
      const int8_t want = m == MH_OCCGRID_NONE ? kGridUnknown : m >= g.l_occ ? kGridOccupied : kGridFree;
      CHECK(g.cells[i] == want);
      n[want == kGridOccupied ? 0 : want == kGridFree ? 1 : 2]++;
    }
    CHECK(g.cells_occupied == n[0] && g.cells_free == n[1] && g.cells_unknown == n[2]);
    // ---- the files
    g.x0 = (int32_t)(rng() % 400) - 200;
    g.y0 = (int32_t)(rng() % 400) - 200;
    g.resolution = trial % 2 ? 0.05 : 0.25;
    const std::string prefix = dir + "/grid" + std::to_string(trial);
    write_occupancy_grid(g, prefix);
    std::string pgm = "P5\n" + std::to_string(g.nx) + " " + std::to_string(g.ny) + "\n255\n";
    for (uint32_t r = 0; r < g.ny; r++)
      for (uint32_t c = 0; c < g.nx; c++) {
        const int8_t v = g.cells[(size_t)(g.ny - 1 - r) * g.nx + c];
        pgm.push_back((char)(v == kGridOccupied ? 0 : v == kGridFree ? 254 : 205));
      }
    CHECK(slurp(prefix + ".pgm") == pgm);
    char yaml[512];
    snprintf(yaml, sizeof(yaml), "image: grid%d.pgm\nresolution: %.9g\norigin: [%.9g, %.9g, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n",
             trial, g.resolution, g.x0 * g.resolution, g.y0 * g.resolution);
    CHECK(slurp(prefix + ".yaml") == yaml);
    const OccupancyGrid back = read_occupancy_grid(prefix);
    CHECK(back.x0 == g.x0 && back.y0 == g.y0 && back.nx == g.nx && back.ny == g.ny && back.resolution == g.resolution);
    CHECK(back.cells == g.cells && back.cells_occupied == n[0] && back.cells_free == n[1] && back.cells_unknown == n[2]);
    CHECK(back.max_logodds.empty());
    if (trial == 0) {  // a truncated image, a foreign byte, a missing file, an unwritable place
      { std::ofstream out(prefix + ".pgm", std::ios::binary | std::ios::trunc); out.write(pgm.data(), (std::streamsize)pgm.size() - 1); }
      CHECK(refuses([&] { (void)read_occupancy_grid(prefix); }));
      pgm.back() = 7;
      { std::ofstream out(prefix + ".pgm", std::ios::binary | std::ios::trunc); out.write(pgm.data(), (std::streamsize)pgm.size()); }
      CHECK(refuses([&] { (void)read_occupancy_grid(prefix); }));
      CHECK(refuses([&] { (void)read_occupancy_grid(dir + "/nowhere"); }));
      CHECK(refuses([&] { write_occupancy_grid(g, dir + "/no_such_dir/grid"); }));
      OccupancyGrid empty;
      CHECK(refuses([&] { write_occupancy_grid(empty, prefix); }));
      OccupancyGrid wrong = g;
      wrong.max_logodds.pop_back();
      CHECK(refuses([&] { occupancy_grid_classify(wrong); }));
    }
  }
  // ---- a set without points is refused before any device is asked for
  molahip_host::KeyFrameSet set;
  CHECK(refuses([&] { (void)build_occupancy_grid(set, d); }));
  set.maps.resize(1);
  set.maps[0].name = "localmap";
  set.maps[0].class_name = "CVoxelMap";
  set.frames.resize(3);
  CHECK(refuses([&] { (void)build_occupancy_grid(set, d); }));
  OccupancyGridOptions other = d;
  other.target_map = "elsewhere";
  CHECK(refuses([&] { (void)build_occupancy_grid(set, other); }));
  printf("ok\n");
  return 0;
}
